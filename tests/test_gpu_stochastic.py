"""Dropout, drop-path and attn_drop against exact-mask float64 references (GPU-only).

The masks are a pure function of (seed, index); tests/stoch_cases.py restates them on the host, so every stochastic op is compared
element for element with a deterministic reference -- no statistics, no exempted elements.  Each check prints a
`STOCH_PARITY <case>: err ... bound ...` line before it asserts (one run is kept in profiles/stochastic_parity.txt).
"""
import numpy as np
import pytest
import torch

import stoch_cases as sc
from conftest import TOL_BF16_FWD, TOL_BF16_GRAD, TOL_BF16_OP, TOL_F32, check_close, rel_err
import metatransformer_amd as M
from metatransformer_amd import ops

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# the bounds the p = 0 attention tests hold (tests/test_gpu_ops.py): forward, backward, lse
ATTN_TOL = {F32: (2e-5, 5e-5, 1e-5), BF16: (1.5e-2, 3e-2, 5e-3)}
# one (batch, head) item against ITS OWN scale: the bounds of test_attention_persistent_kernels_fwd_bwd (0.05 / 0.08, bf16) and the same
# multiples of the global bound for fp32.  An item's scale is floored at a quarter of the global one, so that an item without a scale of
# its own (N = 1: dQ = dK = 0) is still held to 4x these figures of the global scale.
ITEM_TOL = {F32: (7e-5, 1.4e-4), BF16: (0.05, 0.08)}


def _name(dt):
    return "f32" if dt == F32 else "bf16"


def report(case: str, err: float, bound: float) -> float:
    print(f"STOCH_PARITY {case}: err {err:.3e} bound {bound:.1e}")
    return err


def close(got, ref, tol, case):
    """print the figure, then the project's parity check (max-abs bound + per-element bound)"""
    report(case, rel_err(got, ref), tol)
    check_close(got, ref, tol, case)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- a. me_dropout_add

def path_seed(start: int, n_samples: int, p_path: float, want_kept: bool = None) -> int:
    """first seed from `start` whose host drop-path mask drops at least one sample and keeps at least one (one sample: is `want_kept`)"""
    for s in range(start, start + 10000):
        k = sc.path_keep(s, n_samples, p_path)
        if (k.any() and not k.all()) if n_samples > 1 else bool(k[0]) == want_kept:
            return s
    raise AssertionError("no seed found")


# (rows, cols, rows_per_sample): 3 samples of 4 columns (one quad per row); the Block's size (grid-stride loop over > 1 block); 37 samples
# with a column count that is no power of two; ONE sample of 193 quads; a last sample that is cut short by `rows` (335 = 37 * 9 + 2)
DROPOUT_SHAPES = [(21, 4, 7), (64 * 50, 256, 50), (333, 100, 9), (5, 772, 5), (335, 100, 9)]


@pytest.mark.parametrize("vdt,odt", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
@pytest.mark.parametrize("rows,cols,rps", DROPOUT_SHAPES)
def test_dropout_add_exact_mask(dev, rows, cols, rps, vdt, odt):
    n_samples = -(-rows // rps)
    tol = 1e-6 if odt == F32 else TOL_BF16_OP
    v = rnd(rows, cols, seed=rows + cols).to(vdt)
    res = rnd(rows, cols, seed=rows + cols + 1).to(odt)
    cs = 0.5 + torch.rand(cols, generator=torch.Generator().manual_seed(cols))
    g = rnd(rows, cols, seed=rows + cols + 2).to(odt)
    ones = torch.ones(rows, cols, dtype=vdt, device=dev)
    for p_drop in (0.0, 0.25):
        for p_path in (0.0, 0.3):
            # one sample cannot be both dropped and kept: that shape runs once with a seed that drops it and once with one that keeps it
            kinds = (None,) if (p_path == 0 or n_samples > 1) else (False, True)
            for want_kept in kinds:
                seed = path_seed(1000 + rows, n_samples, p_path, want_kept) if p_path > 0 else 1000 + rows
                case = f"dropout_add {rows}x{cols}/{rps} {_name(vdt)}->{_name(odt)} p_drop={p_drop} p_path={p_path} seed={seed}"
                if p_path > 0:
                    pk = sc.path_keep(seed, n_samples, p_path)
                    assert (pk.any() and not pk.all()) if n_samples > 1 else bool(pk[0]) == want_kept
                k32 = torch.from_numpy(sc.dropout_add_scale(seed, rows, cols, rps, p_drop, p_path))      # the kernel's own fp32 factor
                # all-ones input: the output IS the mask scale, bit for bit
                out = ops.dropout_add(ones, None, rps, p_drop, p_path, seed, out_dtype=odt)
                same = torch.equal(out.cpu(), k32.to(odt))
                report(case + " ones", 0.0 if same else float((out.cpu().float() - k32).abs().max()), 0.0)
                assert same, case
                # general: float64 keep * path * colscale * v + res
                k64 = (torch.from_numpy(sc.dropout_keep(seed, rows, cols, p_drop)).double() / (1.0 - float(np.float32(p_drop)))
                       * (torch.from_numpy(np.repeat(sc.path_keep(seed, n_samples, p_path), rps)[:rows]).double()
                          / (1.0 - float(np.float32(p_path))))[:, None])
                out = ops.dropout_add(v.to(dev), res.to(dev), rps, p_drop, p_path, seed, colscale=cs.to(dev))
                assert out.dtype == odt
                close(out, k64 * cs.double() * v.double() + res.double(), tol, case + " general")
                # backward form: the same call on the incoming gradient, res = None -- the same mask
                dg = ops.dropout_add(g.to(dev), None, rps, p_drop, p_path, seed)
                assert dg.dtype == odt
                close(dg, k64 * g.double(), tol, case + " backward")
                assert torch.equal(dg.cpu() == 0, (k32 == 0) | (g == 0)), case + ": zero pattern of the backward form"
                if odt == F32:      # fp32 in and out: one multiplication by the fp32 factor, exact
                    assert torch.equal(dg.cpu(), g * k32), case + ": backward form, fp32"


# ----------------------------------------------------------------------------- b. attention with dropout on the probabilities

# the smallest shapes that cross each boundary of the generic kernels (128 queries per block, 64 keys per tile, head-dim templates
# 32 / 64 / 128): one token; ragged single tiles at head dims 24 (the Graph recipe: 32 heads x 24 at N = 50); exactly one key tile; one
# key past it; one query past a block (129) and two (130) at head dims whose head_dim / 8 is no power of two (40, 48, 56, 72: the scalar
# delta kernel); the 128 template at its full width and at 72 of 128; several key tiles and query blocks with ragged tails
ATTN_SHAPES = [(2, 1, 1, 8), (2, 33, 2, 24), (4, 50, 32, 24), (1, 64, 2, 32), (2, 65, 2, 40), (2, 129, 2, 48), (1, 130, 2, 64),
               (1, 197, 3, 64), (1, 257, 1, 72), (1, 130, 2, 128), (1, 300, 2, 56)]
ATTN_CASES = ([(s, dt, p) for s in ATTN_SHAPES for dt in (F32, BF16) for p in (0.1, 0.5)]
              + [((2, 37, 2, 12), F32, p) for p in (0.1, 0.5)]                      # head_dim % 4 == 0 only: fp32
              + [((1, 257, 1, 72), dt, 0.0) for dt in (F32, BF16)])                 # head_dim 72 is new ground without dropout too


def check_attention(dev, qkv, do, B, N, H, hd, dt, p, seed, case, tols=None):
    """forward and backward of me_attention with dropout p against the float64 reference with the host mask"""
    tol_f, tol_b, tol_l = tols or ATTN_TOL[dt]
    item_f, item_b = ITEM_TOL[dt]
    scale = hd ** -0.5
    C = H * hd
    qr = qkv.double().requires_grad_(True)
    ref, lse_ref = sc.attention_qkv_masked(qr, B, N, H, hd, scale, p, seed)
    ref.backward(do.double())
    ref, lse_ref, gref = ref.detach(), lse_ref.detach(), qr.grad
    out, lse = ops.attention_fwd(qkv.to(dev), B, N, H, hd, scale, True, p_drop=p, seed=seed)
    dqkv = ops.attention_bwd(qkv.to(dev), out, do.to(dev), lse, B, N, H, hd, scale, p_drop=p, seed=seed)
    close(out.float(), ref, tol_f, case + " out")
    report(case + " lse", rel_err(lse, lse_ref), tol_l)
    assert rel_err(lse, lse_ref) < tol_l, case
    whole = float(gref.abs().max())
    for j, nm in enumerate(("dQ", "dK", "dV")):
        got, want = dqkv.float()[:, j * C:(j + 1) * C], gref[:, j * C:(j + 1) * C]
        if float(want.abs().max()) < 1e-3 * whole:       # (N = 1: dQ and dK are identically zero -- no scale of their own)
            err = float((got.cpu().double() - want).abs().max()) / whole
            report(f"{case} {nm} (of the whole gradient's scale)", err, tol_b)
            assert err <= tol_b, (case, nm)
            continue
        close(got, want, tol_b, f"{case} {nm}")

    # every (batch, head) item against its own scale: an item that took another item's mask is far off while the global error stays small
    def items(t, parts):
        return t.detach().double().cpu().reshape(B, N, parts, H, hd).permute(0, 3, 2, 1, 4).reshape(B * H, parts, N * hd)

    for nm, got, want, tol in (("out", items(out, 1), items(ref, 1), item_f), ("dQ/dK/dV", items(dqkv, 3), items(gref, 3), item_b)):
        part = want.abs().amax(dim=(0, 2))                                    # per part (dQ, dK, dV have scales of their own ...
        part = torch.where(part < 1e-3 * part.max(), part.max(), part)        # ... except at N = 1, where dQ = dK = 0: the whole gradient's)
        scale_i = torch.maximum(want.abs().amax(dim=-1), 0.25 * part[None, :])
        worst = ((got - want).abs().amax(dim=-1) / scale_i)
        report(f"{case} per-item {nm}", float(worst.max()), tol)
        assert float(worst.max()) < tol, (case, nm, int(worst.argmax()))
    return out, dqkv


@pytest.mark.parametrize("shape,dt,p", ATTN_CASES, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v).replace(" ", ""))
def test_attention_dropout_exact_mask(dev, shape, dt, p):
    B, N, H, hd = shape
    qkv = rnd(B * N, 3 * H * hd, seed=B * 1000 + N + hd).to(dt)
    do = rnd(B * N, H * hd, seed=77).to(dt)
    seed = 0x9E3779B9 * (N + 1) + hd                     # (beyond 32 bits for most shapes)
    check_attention(dev, qkv, do, B, N, H, hd, dt, p, seed, f"attention {B}x{N}x{H}x{hd} {_name(dt)} p={p}")


@pytest.mark.parametrize("dt", [F32, BF16])
def test_attention_dropout_windowed_call_site(dev, dt):
    """the windowed Block's call: token rows regrouped into B * n_windows items of ws * ws tokens (zero rows where the padded grid
    exceeds the image), attention with dropout on that batch -- the mask is indexed over the WINDOWED batch"""
    B, gh, gw, ws, H, hd, p, seed = 2, 9, 5, 4, 4, 32, 0.1, 0xABCDEF0123
    nwin = -(-gh // ws) * -(-gw // ws)
    qkv = rnd(B * gh * gw, 3 * H * hd, seed=5).to(dt)
    wins = ops.window_rows(qkv.to(dev), B, gh, gw, ws, merge=False)
    assert wins.shape[0] == B * nwin * ws * ws
    do = rnd(B * nwin * ws * ws, H * hd, seed=6).to(dt)
    check_attention(dev, wins.cpu(), do, B * nwin, ws * ws, H, hd, dt, p, seed, f"attention windowed {B}x{gh}x{gw}/{ws} {_name(dt)} p={p}")


# ----------------------------------------------------------------------------- c. mask index width

def test_attention_dropout_mask_index_beyond_32_bits(dev):
    """B * H * N * N = 4.31e9 mask indices: an index truncated to 32 bits (or taken as a signed int) in any of the three kernels gives the
    late items an early item's mask.  One forward and one backward over the whole batch; float64 references and host masks for item 0,
    the items that hold index 2^31 and 2^32, one item between them and the last one."""
    B, H, N, hd, p, seed, dt = 1100, 2, 1400, 8, 0.25, 0x5DEECE66D, BF16
    C = H * hd
    scale = hd ** -0.5
    assert B * H * N * N > 1 << 32
    g = torch.Generator(device=dev).manual_seed(11)
    qkv = torch.randn(B * N, 3 * C, generator=g, device=dev).to(dt)
    do = torch.randn(B * N, C, generator=g, device=dev).to(dt)
    out, lse = ops.attention_fwd(qkv, B, N, H, hd, scale, True, p_drop=p, seed=seed)
    dqkv = ops.attention_bwd(qkv, out, do, lse, B, N, H, hd, scale, p_drop=p, seed=seed)
    items = [0, (1 << 31) // (N * N), (3 << 30) // (N * N), (1 << 32) // (N * N), B * H - 1]
    assert items == [0, 1095, 1643, 2191, 2199]
    assert items[1] * N * N < 1 << 31 < (items[1] + 1) * N * N and items[3] * N * N < 1 << 32 < (items[3] + 1) * N * N
    tol_f, tol_b, tol_l = ATTN_TOL[dt]
    for it, keep in zip(items, sc.attn_keep(seed, B, H, N, p, items=items)):
        b, h = divmod(it, H)
        rows = slice(b * N, (b + 1) * N)
        x = qkv[rows].cpu().double().reshape(N, 3, H, hd)[:, :, h].requires_grad_(True)          # [N, 3, hd]
        factor = torch.from_numpy(keep.astype(np.float64)) / (1.0 - float(np.float32(p)))
        ref, lse_ref = sc.attention_masked(x[:, 0], x[:, 1], x[:, 2], scale, factor)
        ref.backward(do[rows, h * hd:(h + 1) * hd].cpu().double())
        case = f"attention index width item {it} (b={b}, h={h})"
        close(out[rows, h * hd:(h + 1) * hd], ref.detach(), tol_f, case + " out")
        report(case + " lse", rel_err(lse[b, h], lse_ref.detach()), tol_l)
        assert rel_err(lse[b, h], lse_ref.detach()) < tol_l, case
        for j, nm in enumerate(("dQ", "dK", "dV")):
            close(dqkv[rows, j * C + h * hd:j * C + (h + 1) * hd], x.grad[:, j], tol_b, f"{case} {nm}")


# ----------------------------------------------------------------------------- d. a training-mode Block

def block_manual_seed(B: int, p_path: float, start: int):
    """a torch.manual_seed value for which the seed the Block then draws gives host drop-path masks that, per branch, drop at least one
    sample and keep at least one, and that drop BOTH branches of at least one sample"""
    for ms in range(start, start + 10000):
        seed = sc.block_seed(ms)
        if p_path == 0:
            return ms, seed
        k1, k3 = sc.path_keep(seed + sc.SEED_BRANCH1, B, p_path), sc.path_keep(seed + sc.SEED_BRANCH2, B, p_path)
        if all(k.any() and not k.all() for k in (k1, k3)) and (~(k1 | k3)).any():
            return ms, seed
    raise AssertionError("no seed found")


BLOCK_CASES = [
    # (name, dim, heads, Block keywords, (B, N), token grid of a windowed block, autocast)
    ("vit fp32", 128, 2, dict(qkv_bias=True, drop=0.2, drop_path=0.25, attn_drop=0.1), (16, 20), None, False),
    ("vit layer-scale fp32", 128, 2, dict(qkv_bias=True, drop=0.2, drop_path=0.25, attn_drop=0.1, layer_scale=True), (16, 20), None, False),
    ("graph fp32", 768, 32, dict(attn_drop=0.1), (6, 46), None, False),
    ("graph bf16 autocast", 768, 32, dict(attn_drop=0.1), (6, 46), None, True),
    ("windowed fp32", 128, 4, dict(qkv_bias=True, drop=0.2, drop_path=0.25, attn_drop=0.1, windowed=True, window_size=4), (16, 45), (9, 5), False),
]


@pytest.mark.parametrize("name,dim,heads,kw,BN,grid,autocast", BLOCK_CASES, ids=[c[0].replace(" ", "-") for c in BLOCK_CASES])
def test_training_block_matches_masked_oracle(dev, name, dim, heads, kw, BN, grid, autocast):
    """forward, dL/dx and every parameter gradient of a training-mode Block against autograd through block_forward_masked (float64,
    the host's masks); a sample whose two branches are dropped passes through bit for bit, forward and backward"""
    B, N = BN
    p_drop, p_path, p_attn = kw.get("drop", 0.0), kw.get("drop_path", 0.0), kw.get("attn_drop", 0.0)
    torch.manual_seed(17)
    blk = M.Block(dim, heads, **kw).to(dev).train()
    if kw.get("layer_scale"):
        with torch.no_grad():
            blk.gamma1.uniform_(0.2, 1.5); blk.gamma2.uniform_(0.2, 1.5)
    x, go = torch.randn(B, N, dim), torch.randn(B, N, dim)
    ms, seed = block_manual_seed(B, p_path, 100)
    both = np.zeros(B, dtype=bool)
    if p_path > 0:
        k1, k3 = sc.path_keep(seed + sc.SEED_BRANCH1, B, p_path), sc.path_keep(seed + sc.SEED_BRANCH2, B, p_path)
        assert k1.any() and not k1.all() and k3.any() and not k3.all()
        both = ~(k1 | k3)
        assert both.any()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr = x.double().requires_grad_(True)
    y_ref = sc.block_forward_masked(xr, sd, heads, p_drop, p_path, p_attn, seed, gamma1=sd.get("gamma1"), gamma2=sd.get("gamma2"),
                                    window=None if grid is None else grid + (kw["window_size"],))
    (y_ref * go.double()).sum().backward()
    xd = x.to(dev).requires_grad_(True)
    torch.manual_seed(ms)                                # Block.forward draws its seed as the next number of torch's CPU generator
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = blk(xd, *grid) if grid is not None else blk(xd)
    (y * go.to(dev)).sum().backward()
    tol_f, tol_g = (TOL_BF16_FWD, TOL_BF16_GRAD) if autocast else (TOL_F32, TOL_F32)
    case = f"block {name} manual_seed={ms}"
    checks = [("y", y, y_ref, tol_f), ("dx", xd.grad, xr.grad, tol_g)] + [(k, p.grad, sd[k].grad, tol_g) for k, p in blk.named_parameters()]
    assert {k for k, _ in blk.named_parameters()} == set(sd)
    for nm, got, want, tol in checks:
        err = report(f"{case} {nm}", rel_err(got, want), tol)
        assert err < tol, (case, nm)
        if not autocast:      # fp32: per element too (a gradient taken under another mask is wrong in single elements of ordinary size)
            check_close(got, want, tol, f"{case} {nm}")
    for b in np.nonzero(both)[0]:
        assert torch.equal(y[b], xd[b].detach()), (case, "a sample whose two branches are dropped: y == x", int(b))
        assert torch.equal(xd.grad[b], go[b].to(dev)), (case, "a sample whose two branches are dropped: dx == dy", int(b))
