"""Time-Series decoder timing: metatransformer_amd.Decoder (the recipe: d_model 768, 8 heads, d_ff 2048, one layer, c_out 7) next to the
plain-torch restatement of the same decoder (tests/ts_decoder_cases.decoder_torch) with the same parameters on the same GPU.

    python tools/ts_decoder_time.py [--iters 50] [--out profiles/ts_decoder_time.txt]

Shapes: B = 32, cross length S = 96, decoder length L = 48 + pred_len for pred_len in {96, 192, 336, 720} (the recipe's label_len 48).
Forward (no gradient) and forward + backward (gradients for x, cross and every parameter), in fp32 and under bf16 autocast.
Method of tools/graph_tokenizer_time.py: device events around windows of back-to-back calls, each at least 20 ms and at least `iters`
calls long, 5 warm-up calls, the two sides in alternating windows in the same process, median (min-max) of 7 windows.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import metatransformer_amd as M  # noqa: E402
import ts_decoder_cases as tc  # noqa: E402

WINDOW_MS = 20.0
D_MODEL, HEADS, D_FF, LAYERS, C_OUT, BATCH, S_LEN, LABEL = 768, 8, 2048, 1, 7, 32, 96, 48


def calls_per_window(fn, floor):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return max(floor, int(WINDOW_MS / max(e0.elapsed_time(e1) / 5, 1e-3)) + 1)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def timed(fns, floor, windows=7):
    """the given callables in alternating windows -> [(median, min, max)] us per call"""
    n = [calls_per_window(f, floor) for f in fns]
    t = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            t[i].append(window(f, n[i]))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ts_decoder_time.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    keys = tc.decoder_keys(D_MODEL, HEADS, D_FF, LAYERS, C_OUT)
    params = tc.synth_params("timing", keys)
    dec = M.Decoder([M.DecoderLayer(M.AttentionLayer(M.FullAttention(True, 1, attention_dropout=0.1, output_attention=False), D_MODEL, HEADS),
                                    M.AttentionLayer(M.FullAttention(False, 1, attention_dropout=0.1, output_attention=False), D_MODEL, HEADS),
                                    D_MODEL, D_FF, dropout=0.1, activation="gelu") for _ in range(LAYERS)],
                    norm_layer=torch.nn.LayerNorm(D_MODEL), projection=torch.nn.Linear(D_MODEL, C_OUT))
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    dec = dec.to(dev).eval()
    sd = {k: torch.from_numpy(v).to(dev).requires_grad_() for k, v in params.items()}
    lines = [f"# Time-Series decoder, d_model {D_MODEL}, {HEADS} heads, d_ff {D_FF}, {LAYERS} layer, c_out {C_OUT}; B = {BATCH}, S = {S_LEN}, "
             f"L = {LABEL} + pred_len; {torch.cuda.get_device_name(0)}; us per call, median (min-max) of 7 windows of >= {args.iters} calls",
             "# hip = metatransformer_amd.Decoder, torch = the plain-torch restatement (tests/ts_decoder_cases.decoder_torch), alternating windows"]
    for pred in (96, 192, 336, 720):
        L = LABEL + pred
        rnd = lambda what, shape: torch.from_numpy(tc.mc.uniform(shape, tc.mc.seed_of("timing", what, L), -1.0, 1.0, bits=16) * np.float32(1.7)).to(dev)      # noqa: E731
        x, cross, dout = rnd("x", (BATCH, L, D_MODEL)), rnd("cross", (BATCH, S_LEN, D_MODEL)), rnd("dout", (BATCH, L, C_OUT))
        xg, cg = x.clone().requires_grad_(), cross.clone().requires_grad_()
        for mode, autocast in (("fp32", False), ("bf16", True)):
            ctx = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast)      # noqa: E731

            def hip_fwd():
                with torch.no_grad(), ctx():
                    dec(x, cross)

            def torch_fwd():
                with torch.no_grad(), ctx():
                    tc.decoder_torch(x, cross, sd, HEADS, LAYERS)

            def hip_train():
                with ctx():
                    y = dec(xg, cg)
                torch.autograd.grad(y, [xg, cg] + list(dec.parameters()), dout)

            def torch_train():
                with ctx():
                    y = tc.decoder_torch(xg, cg, sd, HEADS, LAYERS)
                torch.autograd.grad(y.float(), [xg, cg] + list(sd.values()), dout)

            (hf, tf), (hb, tb) = timed([hip_fwd, torch_fwd], args.iters), timed([hip_train, torch_train], args.iters)
            fmt = lambda r: f"{r[0]:9.1f} ({r[1]:.1f}-{r[2]:.1f})"      # noqa: E731
            lines.append(f"pred_len {pred:3d} L {L:3d} {mode}  fwd: hip {fmt(hf)} torch {fmt(tf)} ratio {tf[0] / hf[0]:.2f}   "
                         f"fwd+bwd: hip {fmt(hb)} torch {fmt(tb)} ratio {tb[0] / hb[0]:.2f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
