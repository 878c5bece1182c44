"""Time me_fbank on the GPU and record its parity figures.

    python tools/fbank_bench.py [--out-dir profiles] [--iters 200] [--repeats 5]

Writes two files:
  fbank.txt         per shape: the time of one me_fbank call (HIP events around `iters` back-to-back calls through the C ABI, descriptor
                    and workspace made once; best and median of `repeats`), the bytes the call must move (4 bytes per sample in, T x n_mel
                    elements out), the time those bytes take at the measured 6.3 TB/s copy rate, and their ratio; and, for scale, the clips
                    per second of the fp32 CPU restatement (tests/fbank_cases.py) on this host.
  fbank_parity.txt  per case of tests/test_gpu_fbank.py: max |device - restatement in fp64| and e_ref = max |restatement in fp32 - fp64|.
Needs a GPU: there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fbank_cases as fc                      # noqa: E402
import metatransformer_amd as M               # noqa: E402
from metatransformer_amd import _capi         # noqa: E402

COPY_RATE = 6.3e12                            # bytes / s, the measured device-to-device copy rate
SHAPES = [(128, 163840, 16000, 128, 1024, torch.float32), (128, 16000, 16000, 224, 224, torch.float32),
          (128, 163840, 16000, 128, 1024, torch.bfloat16)]


def time_shape(dev, B, n, sr, n_mel, L, odt, iters, repeats):
    lib = _capi.load()
    mod = M.KaldiFbank(sr, n_mel, target_length=L, norm_mean=-4.2677393, norm_std=4.5689974, out_dtype=odt).to(dev)
    wave = 0.1 * torch.randn(B, n, device=dev)
    out = torch.empty(B, L, n_mel, dtype=odt, device=dev)
    d = _capi.FbankDesc()
    d.wave, d.ld_wave, d.B, d.n_samples = wave.data_ptr(), n, B, n
    d.win, d.shift, d.padded, d.n_mel, d.mel_ld, d.target_length = mod.win, mod.shift, mod.padded, n_mel, mod.mel_weight.shape[1], L
    d.window, d.twiddle, d.mel_range, d.mel_weight = mod.window.data_ptr(), mod.twiddle.data_ptr(), mod.mel_range.data_ptr(), mod.mel_weight.data_ptr()
    d.normalize, d.norm_mean, d.norm_std = 1, mod.norm_mean, mod.norm_std
    d.out, d.out_dtype, d.ld_out = out.data_ptr(), _capi.dtype_code(odt), n_mel
    nbytes = lib.me_fbank_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    stream = _capi.stream_ptr()
    call = lambda: _capi.check(lib.me_fbank(ctypes.byref(d), ws.data_ptr(), nbytes, stream), "me_fbank")      # noqa: E731
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    frames = min(mod.num_frames(n), L)
    bytes_in, bytes_out = 4 * B * n, B * L * n_mel * out.element_size()
    floor_ms = (bytes_in + bytes_out) / COPY_RATE * 1e3
    return dict(best=min(ms), median=statistics.median(ms), bytes_in=bytes_in, bytes_out=bytes_out, floor_ms=floor_ms, frames=frames)


def cpu_rate(n, sr, n_mel, L, clips=4):
    waves = [fc.make_wave(n, sr, s) for s in range(clips)]
    fc.fbank(waves[0], sr, n_mel, target_length=L, dtype=torch.float32)
    t0 = time.perf_counter()
    for w in waves:
        fc.fbank(w, sr, n_mel, target_length=L, dtype=torch.float32, norm=(-4.2677393, 4.5689974))
    return clips / (time.perf_counter() - t0)


def parity_lines(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_fbank as tg
    lines = []
    for i, (name, (sr, n_mel)) in enumerate(tg.CONFIGS.items()):
        lengths = tg.clip_lengths(sr)
        wave = tg.batch_of(sr, lengths, 100 * i)
        got = M.KaldiFbank(sr, n_mel).to(dev)(wave.to(dev), torch.tensor(lengths, dtype=torch.int32, device=dev)).cpu()
        for b, n in enumerate(lengths):
            T = fc.num_frames(n, sr)
            if T == 0:
                continue
            r64 = fc.fbank(wave[b, :n], sr, n_mel, dtype=torch.float64)
            r32 = fc.fbank(wave[b, :n], sr, n_mel, dtype=torch.float32)
            e_ref = float((r32.double() - r64).abs().max())
            err = float((got[b, :T].double() - r64).abs().max())
            lines.append(f"{name:8s} len {n:6d} frames {T:3d}   device {err:.3e}   e_ref {e_ref:.3e}   device / e_ref {err / e_ref:5.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fbank_bench.py needs a GPU (timings of anything else say nothing about it)")
    dev = torch.device("cuda:0")
    os.makedirs(a.out_dir, exist_ok=True)
    lines = [f"me_fbank on {torch.cuda.get_device_name(0)}: HIP events around {a.iters} back-to-back calls, best / median of {a.repeats} repeats",
             f"floor = (bytes in + bytes out) / {COPY_RATE / 1e12:.1f} TB/s (the measured copy rate); normalisation on, no masks, no mix-up", ""]
    for B, n, sr, n_mel, L, odt in SHAPES:
        r = time_shape(dev, B, n, sr, n_mel, L, odt, a.iters, a.repeats)
        lines.append(f"wave [{B}, {n}] fp32 at {sr} Hz -> out [{B}, {L}, {n_mel}] {str(odt).replace('torch.', '')} ({r['frames']} frames per clip)")
        lines.append(f"    bytes in {r['bytes_in'] / 1e6:.1f} MB, out {r['bytes_out'] / 1e6:.1f} MB; floor {r['floor_ms'] * 1e3:.1f} us")
        lines.append(f"    me_fbank best {r['best'] * 1e3:.1f} us, median {r['median'] * 1e3:.1f} us = {r['best'] / r['floor_ms']:.1f} x the floor; "
                     f"{B / r['best'] * 1e3:.0f} clips / s")
        print("\n".join(lines[-3:]), flush=True)
    lines.append("")
    for B, n, sr, n_mel, L, odt in SHAPES[:2]:
        rate = cpu_rate(n, sr, n_mel, L)
        lines.append(f"CPU restatement (tests/fbank_cases.py, fp32, torch {torch.__version__}, {torch.get_num_threads()} threads), "
                     f"{n} samples, {n_mel} filters: {rate:.1f} clips / s")
        print(lines[-1], flush=True)
    open(os.path.join(a.out_dir, "fbank.txt"), "w").write("\n".join(lines) + "\n")
    plines = ["me_fbank against tests/fbank_cases.py: max |device - restatement in fp64| and e_ref = max |restatement in fp32 - fp64|,",
              "log domain, per clip of the batches of tests/test_gpu_fbank.py (bound of the test: device <= 4 e_ref)", ""] + parity_lines(dev)
    open(os.path.join(a.out_dir, "fbank_parity.txt"), "w").write("\n".join(plines) + "\n")
    print("\n".join(plines), flush=True)


if __name__ == "__main__":
    main()
