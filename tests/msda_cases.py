"""Inputs of the multi-scale deformable attention fixture (tests/golden/msda.npz), synthesised rather than stored: the fixture
is kept below 1 MB, and the value tensors of these cases alone would take 2 MB and more.  tools/make_msda_golden.py (which runs
the reference on them) and the tests build the same arrays from a counter-based hash (splitmix64 of the element index), so
they do not depend on any library's random stream.  Every value is exact in fp32.

Sample locations are built in pixel space and kept at least 1e-3 from every integer coordinate (the gradient with respect to
a location jumps there), in fp64 and in fp32 arithmetic; `check_clear` verifies it.
"""
from __future__ import annotations

import zlib

import numpy as np

MARGIN = 1e-3


def _mix(n: int, seed: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15 + 0x1234567) % (1 << 64))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def seed_of(*names) -> int:
    return zlib.crc32("/".join(str(n) for n in names).encode())


def uniform(shape, seed: int, lo: float = -1.0, hi: float = 1.0, bits: int = 10) -> np.ndarray:
    """uniform on a grid of 2^bits steps over [lo, hi): exact in fp16 for bits <= 10 and |values| <= 2, always exact in fp32"""
    n = int(np.prod(shape)) if len(shape) else 1
    k = (_mix(n, seed) >> np.uint64(64 - bits)).astype(np.float64)
    return (lo + (hi - lo) * k / float(1 << bits)).astype(np.float32).reshape(shape)


def clear_of_integers(px: np.ndarray) -> np.ndarray:
    """move pixel coordinates closer than 2 MARGIN to an integer to 2 MARGIN beyond it"""
    r = np.round(px)
    d = px - r
    return np.where(np.abs(d) < 2 * MARGIN, r + np.where(d >= 0, 2 * MARGIN, -2 * MARGIN), px)


def pixel_coords(loc: np.ndarray, shapes) -> tuple:
    """(fp64, fp32-arithmetic) pixel coordinates x W - 0.5, y H - 0.5 of loc [..., L, P, 2]"""
    wh = np.array([[w, h] for h, w in shapes], dtype=np.float64)[:, None, :]
    p64 = loc.astype(np.float64) * wh - 0.5
    p32 = (loc.astype(np.float32) * wh.astype(np.float32) - np.float32(0.5)).astype(np.float32)
    return p64, p32


def check_clear(loc: np.ndarray, shapes, what: str = "") -> float:
    p64, p32 = pixel_coords(loc, shapes)
    m = min(float(np.abs(p64 - np.round(p64)).min()), float(np.abs(p32.astype(np.float64) - np.round(p32)).min()))
    assert m >= MARGIN, f"{what}: a sample lies {m:.2e} from a pixel boundary (< {MARGIN})"
    return m


def level_starts(shapes):
    st, s = [], 0
    for h, w in shapes:
        st.append(s)
        s += h * w
    return st, s


# name -> N, Lq, M, D, P, level shapes, location range (normalised) or "pile"
CORE = {
    "injector": dict(N=2, Lq=280, M=12, D=32, P=4, shapes=[(28, 40), (14, 20), (7, 10)], span=(0.0, 1.0)),
    "extractor": dict(N=2, Lq=1470, M=12, D=32, P=4, shapes=[(14, 20)], span=(0.0, 1.0)),
    "d64": dict(N=2, Lq=200, M=6, D=64, P=4, shapes=[(14, 20), (7, 10)], span=(0.0, 1.0)),
    "d20": dict(N=1, Lq=150, M=5, D=20, P=3, shapes=[(9, 13), (5, 6)], span=(0.0, 1.0)),
    "outside": dict(N=2, Lq=240, M=4, D=32, P=4, shapes=[(12, 16), (6, 8)], span=(-0.15, 1.15)),
    "pile": dict(N=2, Lq=280, M=12, D=32, P=4, shapes=[(28, 40), (14, 20), (7, 10)], span="pile"),
}


def core_inputs(name: str) -> dict:
    """value [N, S, M, D], loc [N, Lq, M, L, P, 2], attn [N, Lq, M, L, P] (positive, rows summing to about 1), dout [N, Lq, M D]"""
    c = CORE[name]
    N, Lq, M, D, P, shapes = c["N"], c["Lq"], c["M"], c["D"], c["P"], c["shapes"]
    L = len(shapes)
    starts, S = level_starts(shapes)
    value = uniform((N, S, M, D), seed_of("core", name, "value"))
    dout = uniform((N, Lq, M * D), seed_of("core", name, "dout"))
    attn = uniform((N, Lq, M, L, P), seed_of("core", name, "attn"), 0.0, 2.0 / (L * P), bits=12)
    u = uniform((N, Lq, M, L, P, 2), seed_of("core", name, "loc"), 0.0, 1.0, bits=20).astype(np.float64)
    wh = np.array([[w, h] for h, w in shapes], dtype=np.float64)[:, None, :]
    if c["span"] == "pile":
        # every sample of batch item n inside one 2 x 2 pixel neighbourhood of each level: pixel coordinates in (j, j + 1)
        corner = np.array([[[3.0, 2.0]], [[1.0, 4.0]]])[:N].reshape(N, 1, 1, 1, 1, 2)
        px = corner + 0.02 + 0.96 * u
    else:
        lo, hi = c["span"]
        px = (lo + (hi - lo) * u) * wh - 0.5
    loc = ((clear_of_integers(px) + 0.5) / wh).astype(np.float32)
    check_clear(loc, shapes, f"core/{name}")
    return dict(value=value, loc=loc, attn=attn, dout=dout, shapes=shapes, starts=starts)


# MSDeformAttn module cases: d_model, heads, levels, points, ratio, reference_points width, padding mask
MODULE = {
    "r1_ref2": dict(d_model=96, M=6, P=4, ratio=1.0, shapes=[(12, 16), (6, 8), (3, 4)], q_level=1, ref=2, mask=False, N=2),
    "r05_ref2_mask": dict(d_model=96, M=6, P=4, ratio=0.5, shapes=[(12, 16), (6, 8), (3, 4)], q_level=1, ref=2, mask=True, N=2),
    "r05_ref4": dict(d_model=64, M=4, P=2, ratio=0.5, shapes=[(8, 8), (4, 4)], q_level=0, ref=4, mask=False, N=2),
    "r1_ref4_mask": dict(d_model=64, M=4, P=2, ratio=1.0, shapes=[(8, 8), (4, 4)], q_level=0, ref=4, mask=True, N=1),
}

# fractional part of the sampling-offset biases: with reference points on the pixel centres of one level, the pixel coordinate on
# a level of 2x / 1x / 0.5x that resolution is an integer + {0, 0.5, 0.25, 0.75} + offset, so offsets = bias + (small query term)
# with frac(bias) in [0.08, 0.17] stay clear of every integer
BIAS_FRAC = (0.08, 0.17)
OFFSET_WEIGHT = 2.0 ** -9       # |sampling_offsets.weight| bound: the query-dependent part of an offset stays below ~0.05 pixel


def state_dict_arrays(keys_shapes, tag: str) -> dict:
    """fp16-representable parameters for a [(key, shape)] list: LayerNorm-like weights around 1, sampling-offset weights small
    and biases with the fractional parts of BIAS_FRAC, everything else ~ fan-in scaled"""
    out = {}
    for key, shape in keys_shapes:
        shape = tuple(shape)
        s = seed_of(tag, key)
        leaf = key.rsplit(".", 2)[-2:] if "." in key else [key]
        if "sampling_offsets" in key and key.endswith("weight"):
            a = uniform(shape, s, -OFFSET_WEIGHT, OFFSET_WEIGHT)
        elif "sampling_offsets" in key and key.endswith("bias"):
            whole = np.floor(uniform(shape, s, -2.0, 2.0))
            a = (whole + uniform(shape, s + 1, BIAS_FRAC[0], BIAS_FRAC[1], bits=8)).astype(np.float32)
        elif "norm" in leaf[0] and key.endswith("weight"):
            a = 1.0 + uniform(shape, s, -0.125, 0.125)
        elif key.endswith("gamma") or key.endswith("gamma1") or key.endswith("gamma2"):
            a = uniform(shape, s, 0.25, 0.75)
        elif key.endswith("bias"):
            a = uniform(shape, s, -0.0625, 0.0625)
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            a = uniform(shape, s, -1.0, 1.0) * np.float32(2.0 ** -round(np.log2(max(fan_in, 1)) / 2))
        out[key] = a.astype(np.float16).astype(np.float32)
    return out


def centres(shapes) -> np.ndarray:
    """[sum H W, 2] pixel centres ((j + 0.5) / W, (i + 0.5) / H), levels concatenated"""
    pts = []
    for h, w in shapes:
        ys, xs = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
        pts.append(np.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    return np.concatenate(pts).astype(np.float32)


def module_inputs(name: str) -> dict:
    c = MODULE[name]
    shapes, N, C = c["shapes"], c["N"], c["d_model"]
    L = len(shapes)
    starts, S = level_starts(shapes)
    qh, qw = shapes[c["q_level"]]
    Lq = qh * qw
    ctr = centres([shapes[c["q_level"]]])                                   # [Lq, 2]
    if c["ref"] == 2:
        ref = np.broadcast_to(ctr[None, :, None, :], (N, Lq, L, 2)).copy()
    else:
        # boxes whose half width / n_points is one pixel of the level: loc = centre + offset / W_l
        wh = np.array([[2.0 * c["P"] / w, 2.0 * c["P"] / h] for h, w in shapes], dtype=np.float32)
        ref = np.concatenate([np.broadcast_to(ctr[None, :, None, :], (N, Lq, L, 2)),
                              np.broadcast_to(wh[None, None], (N, Lq, L, 2))], -1).astype(np.float32).copy()
    out = dict(query=uniform((N, Lq, C), seed_of("module", name, "query")), feat=uniform((N, S, C), seed_of("module", name, "feat")),
               ref=ref, dout=uniform((N, Lq, C), seed_of("module", name, "dout")), shapes=shapes, starts=starts, mask=None)
    if c["mask"]:
        out["mask"] = uniform((N, S), seed_of("module", name, "mask"), 0.0, 1.0) < 0.2
    return out


BLOCK = dict(dim=96, num_heads=6, n_points=4, deform_ratio=0.5, with_cffn=True, cffn_ratio=0.25, extra_extractor=True, init_values=0.5,
             H=8, W=12, N=2, vit_heads=3, depth=2)


def block_inputs() -> dict:
    b = BLOCK
    H, W, N, C = b["H"], b["W"], b["N"], b["dim"]
    n = (H // 2) * (W // 2)
    return dict(x=uniform((N, H * W, C), seed_of("block", "x")), c=uniform((N, 21 * n, C), seed_of("block", "c")),
                dx=uniform((N, H * W, C), seed_of("block", "dx")), dc=uniform((N, 21 * n, C), seed_of("block", "dc")),
                image_hw=(16 * H, 16 * W))


def subset_index(numel: int, keep: int = 2048) -> np.ndarray:
    """the flat positions of a tensor that the fixture stores: all of a small tensor, an even stride over a large one"""
    if numel <= keep:
        return np.arange(numel)
    return (np.arange(keep, dtype=np.int64) * numel) // keep
