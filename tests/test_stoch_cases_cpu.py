"""Keeps tests/stoch_cases.py (the host restatement of the dropout / drop-path / attn_drop masks) honest without a GPU."""
import numpy as np
import pytest
import torch

import stoch_cases as sc
from oracle import block_oracle as bo

M64 = (1 << 64) - 1


def splitmix_next(state: int):
    """SplitMix64 (Steele, Lea, Flood 2014) in Python integers: (new state, output)"""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def u01_int(seed: int, idx: int) -> float:
    """u01_hash in Python integers: the (idx + 1)-th SplitMix64 output from state `seed`, top 24 bits"""
    _, z = splitmix_next(((seed & M64) + idx * 0x9E3779B97F4A7C15) & M64)
    return (z >> 40) / 2.0 ** 24


def test_known_answer_is_the_published_splitmix64_stream():
    # the published first three outputs of SplitMix64 from state 0
    state, outs = 0, []
    for _ in range(3):
        state, z = splitmix_next(state)
        outs.append(z)
    assert outs == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = sc.u01(0, np.arange(3, dtype=np.uint64))
    assert u.dtype == np.float32
    assert float(u[0]) == 0xE220A8 / 2 ** 24
    assert [float(v) for v in u] == [(z >> 40) / 2.0 ** 24 for z in outs]
    assert float(sc.u01(0, 0)) == 0xE220A8 / 2 ** 24            # (a scalar index works too)


@pytest.mark.parametrize("seed", [0x8000000000000001, 0xFFFFFFFFFFFFFFFF, -5, -(1 << 63), (1 << 64) - 2, 1234567, (1 << 63) - 1])
def test_wraparound_matches_python_integers(seed):
    idx = np.array([0, 1, 2, 1000, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 12345, 4311999999, (1 << 63) + 7],
                   dtype=np.uint64)
    for off in (0, 1, 2, 3, 4):               # seed + 4 crosses 2^64 for the seeds near the top
        got = sc.u01(seed + off, idx)
        want = [u01_int(seed + off, int(i)) for i in idx]
        assert [float(g) for g in got] == want, (seed, off)
    assert np.array_equal(sc.u01(seed, idx), sc.u01(seed & M64, idx))           # a negative int64 seed is its two's complement
    assert np.array_equal(sc.u01(((seed & M64) + 4) & M64, idx), sc.u01(seed + 4, idx))
    # drop-path stream: seed ^ PATH_XOR of the 64-bit seed
    want = [u01_int((seed & M64) ^ 0xD1B54A32D192ED03, i) >= float(np.float32(0.3)) for i in range(50)]
    assert sc.path_keep(seed, 50, 0.3).tolist() == want


def test_index_formulas():
    B, H, N, p, seed = 3, 2, 5, 0.4, 99
    m = sc.attn_keep(seed, B, H, N, p)
    assert m.shape == (B, H, N, N) and m.dtype == bool
    for b, h, q, k in [(0, 0, 0, 0), (0, 0, 1, 3), (2, 1, 4, 4), (1, 0, 3, 1), (2, 0, 0, 2)]:
        assert bool(m[b, h, q, k]) == (u01_int(seed, ((b * H + h) * N + q) * N + k) >= float(np.float32(p)))
    assert np.array_equal(sc.attn_keep(seed, B, H, N, p, items=[5, 0, 3]), m.reshape(B * H, N, N)[[5, 0, 3]])
    assert not np.array_equal(m[0, 0], m[0, 0].T)               # (q, k) is not (k, q)
    d = sc.dropout_keep(seed, 7, 12, p)
    assert d.shape == (7, 12)
    for r, c in [(0, 0), (6, 11), (3, 4)]:
        assert bool(d[r, c]) == (u01_int(seed, r * 12 + c) >= float(np.float32(p)))
    # an index beyond 2^32 (the item that holds it is built without the ones before it)
    big = sc.attn_keep(seed, 1100, 2, 1400, 0.25, items=[2199])
    for q, k in [(0, 0), (1399, 1399), (700, 3)]:
        assert bool(big[0, q, k]) == (u01_int(seed, (2199 * 1400 + q) * 1400 + k) >= 0.25)
    # p = 0 keeps everything, the factor in the kernel's fp32 arithmetic
    assert sc.dropout_keep(seed, 4, 4, 0.0).all() and sc.path_keep(seed, 9, 0.0).all()
    s = sc.dropout_add_scale(seed, 10, 4, 3, 0.25, 0.3)
    pk = sc.path_keep(seed, 4, 0.3)
    dk = sc.dropout_keep(seed, 10, 4, 0.25)
    full = np.float32(np.float32(1) / np.float32(0.7)) * np.float32(np.float32(1) / np.float32(0.75))
    for r in range(10):
        for c in range(4):
            assert s[r, c] == (full if (pk[r // 3] and dk[r, c]) else np.float32(0)), (r, c)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_kept_fraction_within_four_sigma(p):
    def check(mask, what):
        n = mask.size
        assert n >= 10 ** 6
        sigma = (p * (1 - p) / n) ** 0.5
        assert abs(float(mask.mean()) - (1 - p)) <= 4 * sigma, (what, float(mask.mean()), sigma)
    check(sc.attn_keep(2024, 2, 2, 512, p), "attention")
    check(sc.dropout_keep(2025, 1024, 1024, p), "dropout")
    check(sc.path_keep(2026, 10 ** 6, p), "drop-path")


def _block(dim, heads, layer_scale, seed):
    sd = {k[2:]: v.double() for k, v in bo.make_encoder_state_dict(1, dim, seed=seed).items()}
    g = torch.Generator().manual_seed(seed)
    g1 = g2 = None
    if layer_scale:
        g1, g2 = (0.2 + torch.rand(dim, generator=g, dtype=torch.float64) for _ in range(2))
    return sd, g1, g2


@pytest.mark.parametrize("layer_scale", [False, True])
@pytest.mark.parametrize("window", [None, (5, 3, 2)])
def test_block_forward_masked_without_masks_is_the_block_oracle(layer_scale, window):
    sd, g1, g2 = _block(32, 2, layer_scale, 3)
    N = 15 if window is not None else 11
    x = torch.randn(3, N, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got = sc.block_forward_masked(x, sd, 2, 0.0, 0.0, 0.0, 12345, gamma1=g1, gamma2=g2, window=window)
    want = bo.block_forward(x, sd, 2, gamma1=g1, gamma2=g2, window=window)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_block_forward_masked_applies_each_mask_and_is_differentiable():
    dim, heads, B, N = 32, 2, 8, 6
    sd, g1, g2 = _block(dim, heads, True, 4)
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    x = torch.randn(B, N, dim, generator=torch.Generator().manual_seed(2), dtype=torch.float64).requires_grad_(True)
    seed = next(s for s in range(100) if (~(sc.path_keep(s + 1, B, 0.5) | sc.path_keep(s + 3, B, 0.5))).any())
    both = ~(sc.path_keep(seed + 1, B, 0.5) | sc.path_keep(seed + 3, B, 0.5))
    assert both.any()
    y = sc.block_forward_masked(x, sd, heads, 0.2, 0.5, 0.1, seed, gamma1=g1, gamma2=g2)
    for b in np.nonzero(both)[0]:
        assert torch.equal(y[b], x[b])                        # both branches dropped: the sample passes through
    y.sum().backward()
    assert x.grad is not None and all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in sd.values())
    for b in np.nonzero(both)[0]:
        assert torch.equal(x.grad[b], torch.ones_like(x.grad[b]))
    # every probability matters: changing one of them changes the result, the same seed reproduces it
    base = sc.block_forward_masked(x, sd, heads, 0.2, 0.5, 0.1, seed, gamma1=g1, gamma2=g2)
    assert torch.equal(base, y)
    for args in [(0.0, 0.5, 0.1), (0.2, 0.0, 0.1), (0.2, 0.5, 0.0)]:
        assert not torch.equal(sc.block_forward_masked(x, sd, heads, *args, seed, gamma1=g1, gamma2=g2), y)
    assert not torch.equal(sc.block_forward_masked(x, sd, heads, 0.2, 0.5, 0.1, seed + 1, gamma1=g1, gamma2=g2), y)


def test_block_seed_is_the_first_draw_after_manual_seed():
    s = sc.block_seed(5)
    torch.manual_seed(5)
    assert s == int(torch.empty((), dtype=torch.int64).random_().item()) and 0 <= s < 1 << 63
    assert sc.block_seed(6) != s
