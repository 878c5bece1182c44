"""Cases and float64 restatements for the Q/K/V attention kernels (csrc/attention_qkv.hip) and the Time-Series decoder built on them
(metatransformer_amd/timeseries.py).  Shared by tests/test_gpu_attention_qkv.py, tests/test_gpu_ts_decoder.py,
tests/test_ts_decoder_cpu.py and tools/make_ts_decoder_golden.py.  Inputs and parameters are synthesised from seeds
(msda_cases.uniform: a counter hash, exact in fp32), never stored.

The kernels tile 128 queries per block (32 per wave) against 64-key LDS tiles; the shape lists hold the smallest sizes that cross
each of those edges, `assert_coverage` says which property each list must have.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import msda_cases as mc
import stoch_cases as sc

WAVE_ROWS, KEY_TILE, BLOCK_ROWS = 32, 64, 128

# ---------------------------------------------------------------------------------------------------- attention_qkv
QKV_B, QKV_H = 2, 3
QKV_NONCAUSAL = [(1, 1), (33, 1), (1, 65), (31, 63), (64, 64), (129, 65), (144, 96), (70, 17)]       # (Nq, Nk)
QKV_CAUSAL = [1, 31, 64, 65, 129, 144, 200]
QKV_HEAD_DIMS = {torch.float32: [4, 8, 24, 64, 96, 128], torch.bfloat16: [8, 24, 64, 96, 128]}
QKV_LAYOUTS = ["packed3", "q_kv2", "separate_padded"]
QKV_CAUSALITY_N, QKV_CAUSALITY_T = 144, [0, 63, 64, 100]
# (Nq, Nk, causal, head_dim), each in both dtypes, p = 0.1
QKV_DROPOUT = [(33, 65, False, 24), (65, 65, True, 24), (129, 129, True, 96), (70, 17, False, 64)]
QKV_EQUIV = [(64, 24), (129, 64), (200, 128)]                                                         # (N, head_dim) against me_attention_*


def _tiles(n: int, t: int) -> int:
    return -(-n // t)


def assert_coverage() -> None:
    nc, ca = QKV_NONCAUSAL, QKV_CAUSAL
    every_n = [n for pair in nc for n in pair] + ca
    assert any(n % WAVE_ROWS for n in every_n), "an N that is no multiple of the 32 rows of a wave"
    assert any(n % WAVE_ROWS for n in ca) and any(n % WAVE_ROWS == 0 for n in ca)
    for edge in (KEY_TILE, BLOCK_ROWS):                      # sizes on both sides of a key tile and of a query block, and on the edge or next to it
        assert any(n <= edge for n in ca) and any(n > edge for n in ca), edge
        assert any(n <= edge for n, _ in nc) and any(n > edge for n, _ in nc), edge
        assert any(abs(n - edge) <= 1 for n in ca), edge
    assert any(n > KEY_TILE for _, n in nc) and any(n <= KEY_TILE for _, n in nc)
    # Nq on the other side of a tile edge from Nk, both ways
    assert any(_tiles(a, KEY_TILE) > _tiles(b, KEY_TILE) for a, b in nc) and any(_tiles(a, KEY_TILE) < _tiles(b, KEY_TILE) for a, b in nc)
    assert any(a == 1 for a, _ in nc) and any(b == 1 for _, b in nc) and 1 in ca
    assert any(_tiles(n, BLOCK_ROWS) > 1 for n in ca) and any(_tiles(a, BLOCK_ROWS) > 1 for a, _ in nc), "more than one block"
    assert any(_tiles(n, KEY_TILE) >= 4 for n in ca), "a causal case whose last block skips no tile and whose first skips two"
    for dt, hds in QKV_HEAD_DIMS.items():                    # every instantiated width (32, 64, 128), on and below it, and the recipe's 96
        for lo, hi in ((0, 32), (32, 64), (64, 128)):
            assert any(lo < h <= hi for h in hds), (dt, hi)
        assert 96 in hds and 128 in hds and min(hds) == (4 if dt == torch.float32 else 8)
    assert set(QKV_CAUSALITY_T) >= {0, KEY_TILE - 1, KEY_TILE} and QKV_CAUSALITY_N > max(QKV_CAUSALITY_T)
    # dropout: both variants; a causal case past a key tile and a query block at a head_dim above 64 (the HD 128 instantiations, both
    # fp32 dK / dV launches); every instantiated width; head_dims that both dtypes take
    dr = QKV_DROPOUT
    assert any(c for _, _, c, _ in dr) and any(not c and a != b for a, b, c, _ in dr)
    assert any(c and a > BLOCK_ROWS and b > KEY_TILE and hd > 64 for a, b, c, hd in dr)
    for lo, hi in ((0, 32), (32, 64), (64, 128)):
        assert any(lo < hd <= hi for _, _, _, hd in dr), hi
    assert all(hd % 8 == 0 for _, _, _, hd in dr)


def qkv_cases(dt: torch.dtype):
    """[(Nq, Nk, causal, head_dim, layout)]: every shape once, with head_dim and layout rotating; then every head_dim x layout at one
    ragged multi-block shape of each variant"""
    hds = QKV_HEAD_DIMS[dt]
    shapes = [(a, b, False) for a, b in QKV_NONCAUSAL] + [(n, n, True) for n in QKV_CAUSAL]
    out = [(a, b, c, hds[i % len(hds)], QKV_LAYOUTS[i % 3]) for i, (a, b, c) in enumerate(shapes)]
    for a, b, c in ((129, 65, False), (129, 129, True)):
        for hd in hds:
            for lay in QKV_LAYOUTS:
                if (a, b, c, hd, lay) not in out:
                    out.append((a, b, c, hd, lay))
    return out


def qkv_case_id(case) -> str:
    a, b, c, hd, lay = case
    return f"{'causal' if c else 'full'}-{a}x{b}-hd{hd}-{lay}"


def qkv_values(B: int, Nq: int, Nk: int, H: int, hd: int, dt: torch.dtype, seed: int):
    """q [B*Nq, C], k, v [B*Nk, C], dout [B*Nq, C] in dtype dt (CPU); scores of a few units so the softmax is neither flat nor one-hot"""
    C = H * hd
    mk = lambda name, rows: torch.from_numpy(mc.uniform((rows, C), mc.seed_of("qkv", name, seed, rows, C), -1.0, 1.0)).to(dt)
    q, k, v, do = mk("q", B * Nq), mk("k", B * Nk), mk("v", B * Nk), mk("do", B * Nq)
    return (q * 2.0).to(dt), (k * 2.0).to(dt), v, do


def qkv_place(layout: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dev, fill: float = 0.0):
    """the operands as device VIEWS in the named layout (-> (q, k, v) views with the given values) -- and, with the same call on empty
    gradients, where the backward writes.  packed3 needs as many query as key rows."""
    C = q.shape[1]
    pad = 8
    if layout == "packed3":
        buf = torch.full((q.shape[0], 3 * C), fill, dtype=q.dtype, device=dev)
        views = (buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:])
    elif layout == "q_kv2":
        qb = torch.full((q.shape[0], C), fill, dtype=q.dtype, device=dev)
        kv = torch.full((k.shape[0], 2 * C), fill, dtype=q.dtype, device=dev)
        views = (qb, kv[:, :C], kv[:, C:])
    else:
        views = tuple(torch.full((t.shape[0], C + pad), fill, dtype=q.dtype, device=dev)[:, :C] for t in (q, k, v))
    for dst, src in zip(views, (q, k, v)):
        dst.copy_(src)
    return views


def qkv_layout_for(layout: str, Nq: int, Nk: int) -> str:
    return "q_kv2" if layout == "packed3" and Nq != Nk else layout


def qkv_keep(seed: int, B: int, H: int, Nq: int, Nk: int, p: float) -> np.ndarray:
    """keep mask of the probabilities of me_attention_qkv_*: bool [B, H, Nq, Nk], index ((b*H + h)*Nq + q)*Nk + k"""
    idx = np.arange(B * H * Nq * Nk, dtype=np.uint64).reshape(B, H, Nq, Nk)
    return sc.u01(seed, idx) >= np.float32(p)


def qkv_ref(q, k, v, B: int, Nq: int, Nk: int, H: int, hd: int, scale: float, causal: bool, factor: Optional[torch.Tensor] = None):
    """float64: (out [B*Nq, C], lse [B, H, Nq]); factor [B, H, Nq, Nk] multiplies the normalised probabilities (dropout)"""
    q4 = q.double().reshape(B, Nq, H, hd).transpose(1, 2)
    k4 = k.double().reshape(B, Nk, H, hd).transpose(1, 2)
    v4 = v.double().reshape(B, Nk, H, hd).transpose(1, 2)
    s = (q4 @ k4.transpose(-2, -1)) * scale
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Nq, Nk, dtype=torch.bool), diagonal=1), float("-inf"))
    a = torch.softmax(s, dim=-1)
    if factor is not None:
        a = a * factor
    return (a @ v4).transpose(1, 2).reshape(B * Nq, H * hd), torch.logsumexp(s, dim=-1)


# ---------------------------------------------------------------------------------------------------- decoder / timeF embedding
# (B, L, S, d_model, H, d_ff, layers, c_out): the recipe; two layers with ragged L != S; one token; S below a key tile, L above
DECODER_CASES = {
    "recipe": (2, 144, 96, 768, 8, 2048, 1, 7),
    "two_layers": (2, 33, 65, 192, 2, 256, 2, 7),
    "one_token": (1, 1, 1, 96, 1, 128, 1, 3),
    "short_cross": (2, 70, 17, 64, 2, 128, 1, 5),
}
# (B, L, c_in, d_model, freq)
EMBED_CASES = {"hourly": (2, 33, 7, 192, "h"), "minutely": (1, 70, 3, 64, "t")}
D_INP = {"h": 4, "t": 5, "s": 6, "m": 1, "a": 1, "w": 2, "d": 3, "b": 3}
KEEP = 512                                     # positions of a tensor the fixture stores (msda_cases.subset_index)


def decoder_keys(d_model: int, H: int, d_ff: int, layers: int, c_out: int):
    """[(key, shape)] of a Decoder in the reference's registration order"""
    ks = []
    for i in range(layers):
        for att in ("self_attention", "cross_attention"):
            for pr in ("query", "key", "value", "out"):
                ks += [(f"layers.{i}.{att}.{pr}_projection.weight", (d_model, d_model)), (f"layers.{i}.{att}.{pr}_projection.bias", (d_model,))]
        ks += [(f"layers.{i}.conv1.weight", (d_ff, d_model, 1)), (f"layers.{i}.conv1.bias", (d_ff,)),
               (f"layers.{i}.conv2.weight", (d_model, d_ff, 1)), (f"layers.{i}.conv2.bias", (d_model,))]
        for n in (1, 2, 3):
            ks += [(f"layers.{i}.norm{n}.weight", (d_model,)), (f"layers.{i}.norm{n}.bias", (d_model,))]
    return ks + [("norm.weight", (d_model,)), ("norm.bias", (d_model,)), ("projection.weight", (c_out, d_model)), ("projection.bias", (c_out,))]


def synth_params(tag: str, keys):
    """{key: float32 array}: matrices uniform in +-sqrt(3 / fan_in) (unit-variance outputs), LayerNorm weights around 1, other vectors small"""
    out = {}
    for k, shape in keys:
        sd = mc.seed_of("tsdec", tag, k)
        if len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            out[k] = mc.uniform(shape, sd, -1.0, 1.0, bits=16) * np.float32(np.sqrt(3.0 / fan_in))
        elif "norm" in k and k.endswith("weight"):
            out[k] = np.float32(1.0) + np.float32(0.25) * mc.uniform(shape, sd, -1.0, 1.0, bits=16)
        else:
            out[k] = np.float32(0.25) * mc.uniform(shape, sd, -1.0, 1.0, bits=16)
    return out


def decoder_inputs(name: str):
    """x [B, L, d], cross [B, S, d], dout [B, L, c_out] (float32 arrays)"""
    B, L, S, d, H, ff, nl, co = DECODER_CASES[name]
    u = lambda what, shape: mc.uniform(shape, mc.seed_of("tsdec", name, what), -1.0, 1.0, bits=16) * np.float32(1.7)      # noqa: E731
    return u("x", (B, L, d)), u("cross", (B, S, d)), u("dout", (B, L, co))


def embed_keys(c_in: int, d_model: int, freq: str):
    return [("value_embedding.tokenConv.weight", (d_model, c_in, 3)), ("temporal_embedding.embed.weight", (d_model, D_INP[freq]))]


def embed_inputs(name: str):
    """x [B, L, c_in], x_mark [B, L, d_inp] in [-0.5, 0.5] (the range of the reference's time features), dout [B, L, d]"""
    B, L, c_in, d, freq = EMBED_CASES[name]
    u = lambda what, shape, s: mc.uniform(shape, mc.seed_of("tsemb", name, what), -1.0, 1.0, bits=16) * np.float32(s)      # noqa: E731
    return u("x", (B, L, c_in), 1.7), u("mark", (B, L, D_INP[freq]), 0.5), u("dout", (B, L, d), 1.0)


def stored(a64: np.ndarray) -> np.ndarray:
    """what the fixture keeps of a float64 tensor: its KEEP subset positions followed by the element of largest magnitude"""
    a = np.asarray(a64, dtype=np.float64).reshape(-1)
    return a[np.append(mc.subset_index(a.size, KEEP), int(np.abs(a).argmax()))]


def picked(t: torch.Tensor, argmax: int) -> np.ndarray:
    """the same positions of a result, `argmax` taken from the fixture"""
    a = t.detach().double().cpu().numpy().reshape(-1)
    return a[np.append(mc.subset_index(a.size, KEEP), int(argmax))]


def _keep_factor(seed: int, rows: int, cols: int, p: float, like: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(sc.dropout_keep(seed, rows, cols, p).astype(np.float64) / (1.0 - float(np.float32(p)))).to(like)


def decoder_torch(x, cross, sd, H: int, layers: int, p: float = 0.0, p_attn: float = 0.0, seed: int = 0, offsets=None, project: bool = True):
    """The decoder restated in plain torch (Transformer_EncDec.py:98-135 with FullAttention and AttentionLayer written out), in whatever
    dtype / autocast state the caller sets up; differentiable.  sd: {key: tensor} with the reference's keys.  p / p_attn > 0: training
    mode with the EXACT masks of the product -- layer i, site s uses seed + i * offsets['stride'] + offsets[s] (the module's SEED_*
    constants), layer dropouts indexed r * cols + c, attention probabilities ((b*H + h)*L + q)*S + k."""
    import torch.nn.functional as F
    B, L, d = x.shape
    S = cross.shape[1]
    hd = d // H

    def attention(pre, xq, xkv, causal, sd_attn):
        Nk = xkv.shape[1]
        q = F.linear(xq, sd[pre + "query_projection.weight"], sd[pre + "query_projection.bias"]).view(B, L, H, hd).transpose(1, 2)
        k = F.linear(xkv, sd[pre + "key_projection.weight"], sd[pre + "key_projection.bias"]).view(B, Nk, H, hd).transpose(1, 2)
        v = F.linear(xkv, sd[pre + "value_projection.weight"], sd[pre + "value_projection.bias"]).view(B, Nk, H, hd).transpose(1, 2)
        s = (q @ k.transpose(-2, -1)) * (hd ** -0.5)
        if causal:
            s = s.masked_fill(torch.triu(torch.ones(L, Nk, dtype=torch.bool, device=x.device), diagonal=1), float("-inf"))
        a = torch.softmax(s, dim=-1)
        if p_attn > 0:
            a = a * torch.from_numpy(qkv_keep(sd_attn, B, H, L, Nk, p_attn).astype(np.float64) / (1.0 - float(np.float32(p_attn)))).to(a)
        o = (a @ v).transpose(1, 2).reshape(B, L, d)
        return F.linear(o, sd[pre + "out_projection.weight"], sd[pre + "out_projection.bias"])

    def drop(t, sd_site):
        if p <= 0:
            return t
        return t * _keep_factor(sd_site, B * L, t.shape[-1], p, t).reshape(t.shape)

    for i in range(layers):
        pre = f"layers.{i}."
        base = seed + i * offsets["stride"] if offsets else 0
        at = (lambda s: base + offsets[s]) if offsets else (lambda s: 0)
        ln = lambda n, t: F.layer_norm(t, (d,), sd[pre + f"norm{n}.weight"], sd[pre + f"norm{n}.bias"], 1e-5)      # noqa: E731
        x = ln(1, x + drop(attention(pre + "self_attention.", x, x, True, at("self_attn")), at("self_branch")))
        x = ln(2, x + drop(attention(pre + "cross_attention.", x, cross, False, at("cross_attn")), at("cross_branch")))
        y = drop(F.gelu(F.linear(x, sd[pre + "conv1.weight"].squeeze(-1), sd[pre + "conv1.bias"])), at("mlp_hidden"))
        y = drop(F.linear(y, sd[pre + "conv2.weight"].squeeze(-1), sd[pre + "conv2.bias"]), at("mlp_branch"))
        x = ln(3, x + y)
    if not project:
        return x
    x = F.layer_norm(x, (d,), sd["norm.weight"], sd["norm.bias"], 1e-5)
    return F.linear(x, sd["projection.weight"], sd["projection.bias"])
