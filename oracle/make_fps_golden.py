"""Write tests/golden/fps_reference.npz: the indices the REFERENCE'S OWN furthest-point-sampling kernel returns on the seeded
clouds of tests/test_gpu_pointcloud_ref.py.  TEST INFRASTRUCTURE.

    python -m oracle.make_fps_golden            # (re)write the fixture   (needs a GPU and oracle/_ref/libref_fps.so)
    python -m oracle.make_fps_golden --check    # compare the kernel with the stored fixture, write nothing

The kernel is the one oracle/build_ref.py compiles (sampling_gpu.cu, launched by its own launcher on the default stream).
The clouds are not stored: fps_clouds() regenerates them from their seed, and every case keeps the float64 sum of its cloud
so that a drifting generator is caught instead of comparing against indices of other points.
"""
from __future__ import annotations

import argparse
import ctypes
import os

import numpy as np
import torch

from . import build_ref

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fps_reference.npz")

# (n points, m samples, cloud seed, clouds kept): ties, lattices, the block sizes opt_n_threads picks, the S3DIS cloud size,
# and one n beyond the register-resident form of me_fps (24 576 points)
INDEX_CASES = [(n, m, 100 + n, 4) for n, m in ((2, 2), (5, 5), (33, 20), (64, 64), (100, 50), (777, 100), (1024, 256), (2048, 512),
                                                (3000, 64), (8192, 300), (24000, 1500))] + [(30000, 200, 7, 3)]
# the clouds on which oracle.tokenizer_oracle.fps_reference is held to the kernel
LITERAL_CASES = [(n, m, 300 + n, 4) for n, m in ((100, 40), (777, 60), (1500, 48))]


def fps_clouds(n: int, seed: int) -> torch.Tensor:
    """four [n, 3] clouds: uniform, exact duplicates (ties in every round), a coarse lattice (many equal distances, exact
    arithmetic), large coordinates (rounding of the distance decides)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(4, n, 3, generator=g) * 2 - 1
    p[1, n // 2:] = p[1, : n - n // 2].clone()
    p[2] = torch.round(p[2] * 4) / 4
    p[3] = p[3] * 1e3
    return p


def case_key(n: int, m: int, seed: int) -> str:
    return f"n{n}_m{m}_s{seed}"


def load_kernel():
    """the reference launcher as a function (points [B, n, 3] float32 on the GPU, m) -> int32 indices [B, m]"""
    lib = ctypes.CDLL(build_ref.OUT)
    fn = getattr(lib, build_ref.LAUNCHER)
    fn.restype = None
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(p: torch.Tensor, m: int) -> torch.Tensor:
        B, n, _ = p.shape
        idx = torch.zeros(B, m, dtype=torch.int32, device=p.device)
        temp = torch.full((B, n), 1e10, dtype=torch.float32, device=p.device)      # subsample.py:96 fill_(1e10)
        torch.cuda.synchronize()
        fn(B, n, m, p.data_ptr(), temp.data_ptr(), idx.data_ptr())                 # default stream, as the reference launches it
        torch.cuda.synchronize()
        return idx
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if not build_ref.available():
        raise SystemExit("oracle/_ref/libref_fps.so is not built (python -m oracle.build_ref where the reference tree is)")
    if not torch.cuda.is_available():
        raise SystemExit("the reference kernel needs a GPU")
    run = load_kernel()
    out = {}
    for n, m, seed, keep in INDEX_CASES + LITERAL_CASES:
        p = fps_clouds(n, seed)[:keep].contiguous()
        k = case_key(n, m, seed)
        out[k + "/idx"] = run(p.cuda(), m).cpu().numpy()
        out[k + "/cloud_sum"] = np.float64(p.double().sum())
    if args.check:
        z = np.load(GOLDEN)
        bad = [k for k, v in out.items() if not np.array_equal(z[k], v)]
        raise SystemExit(f"differs from {GOLDEN}: {bad}" if bad else 0)
    np.savez(GOLDEN, **out)
    print("wrote", GOLDEN, sum(v.nbytes for v in out.values()) // 1024, "KiB")


if __name__ == "__main__":
    main()
