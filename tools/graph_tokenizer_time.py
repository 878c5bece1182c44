"""Graph tokenizer timing: GraphFeatureTokenizer (one GEMM over the node rows + me_graph_tokens_fwd / _bwd) next to the same
parameters through a PyTorch composition of the same operations on the same GPU (embedding sums, boolean-mask scatters into the
padded batch, the [B, T, 2D] index embeddings through the identifier Linears, type embedding, special tokens, masked_fill).

    python tools/graph_tokenizer_time.py [--iters 20] [--out PATH] [--rev LABEL]

Batches: B = 128 molecule-like graphs (10 to 25 nodes, twice as many directed edges, 9 / 3 feature columns drawn from a few
common values per column), and the pile-up batch (the same graphs, every node one atom value, every edge one edge value).
Configurations: the PCQM4Mv2 recipe (lap k = 16, type id, C = 768) and the Data2Seq default widths (rand + orf at D = 768, lap,
type id).  Identifiers are fixed (node_ids) on both sides.  Method of tools/msda_time.py: device events around windows of
back-to-back calls, each at least 20 ms and `iters` calls long, 5 warm-up calls, the two sides in alternating windows, median
(min-max) of 7 windows.  Split (HIP side, each its own windows): identifier GEMM (with the operand packing) / assembly kernel /
backward index build / backward gathers.
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metatransformer_amd as M  # noqa: E402
from metatransformer_amd import _capi, data2seq  # noqa: E402

WINDOW_MS = 20.0


def calls_per_window(fn, floor):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return max(floor, int(WINDOW_MS / max(e0.elapsed_time(e1) / 10, 1e-3)) + 1)


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


def make_batch(dev, pile, B=128, seed=3):
    g = torch.Generator().manual_seed(seed)
    node_num = torch.randint(10, 26, (B,), generator=g).tolist()
    edge_num = [2 * n for n in node_num]
    Sn, Se = sum(node_num), sum(edge_num)
    # a few common values per feature column, as molecule features have
    node_data = torch.randint(0, 6, (Sn, 9), generator=g) + 1 + 512 * torch.arange(9)
    edge_data = torch.randint(0, 4, (Se, 3), generator=g) + 1 + 512 * torch.arange(3)
    if pile:
        node_data[:], edge_data[:] = 7, 3
    ei = torch.cat([torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
                    for n, e in zip(node_num, edge_num)], dim=1)
    return dict(node_data=node_data.to(dev), edge_data=edge_data.to(dev), edge_index=ei.to(dev), node_num=node_num, edge_num=edge_num,
                lap_eigvec=torch.randn(Sn, 16, generator=g).to(dev), lap_eigval=None, in_degree=None, out_degree=None)


def composition(tok, bd, ids):
    """the tokenizer as PyTorch operations: what a user composes without the kernels"""
    node_num, edge_num = bd["node_num"], bd["edge_num"]
    dev = bd["node_data"].device
    B, max_n = len(node_num), max(node_num)
    T = max(n + e for n, e in zip(node_num, edge_num))
    nn_ = torch.tensor(node_num, device=dev)[:, None]
    en_ = torch.tensor(edge_num, device=dev)[:, None]
    pos = torch.arange(T, device=dev)[None, :]
    is_node, is_edge = pos < nn_, (pos >= nn_) & (pos < nn_ + en_)
    node_mask = is_node[:, :max_n]
    local = torch.arange(max_n, device=dev)[None, :].expand(B, max_n)[node_mask]
    index = torch.zeros(B, T, 2, dtype=torch.long, device=dev)
    index[is_node] = torch.stack([local, local], 1)
    index[is_edge] = bd["edge_index"].t()
    feat = torch.zeros(B, T, tok.encoder_embed_dim, device=dev)
    feat[is_node] = F.embedding(bd["node_data"], tok.atom_encoder.weight).sum(-2)
    feat[is_edge] = F.embedding(bd["edge_data"], tok.edge_encoder.weight).sum(-2)
    for kind, p, w in ids:
        padded = torch.zeros(B, max_n, p.shape[1], device=dev)
        padded[node_mask] = p
        pair = padded[:, :, None, :].expand(B, max_n, 2, p.shape[1]).gather(1, index[..., None].expand(B, T, 2, p.shape[1]))
        feat = feat + F.linear(pair.reshape(B, T, -1), w)
    if tok.type_id:
        feat = feat + F.embedding((index[..., 0] == index[..., 1]).long(), tok.order_encoder.weight)
    special = torch.cat([tok.graph_token.weight, tok.null_token.weight])[None].expand(B, 2, -1)
    feat = torch.cat([special, feat], 1)
    mask = torch.cat([torch.zeros(B, 2, dtype=torch.bool, device=dev), pos >= nn_ + en_], 1)
    return feat.masked_fill(mask[..., None], 0.0), mask, index


def split(tok, bd, ids, node_ids, floor):
    """identifier GEMM / assembly kernel / backward index build / backward gathers, through the C ABI"""
    lib = _capi.load()
    Sn = sum(bd["node_num"])
    with torch.no_grad():
        Z = tok._project(ids, Sn)
    out, mask, idx = tok(bd, node_ids=node_ids)
    fn = out.grad_fn
    node_data, edge_data, edge_index, offsets, atom, edge, gt, nt = fn.saved_tensors
    dims, _ = fn.meta
    dev = out.device
    dout = torch.randn_like(out)
    d = data2seq._graph_desc(node_data, edge_data, edge_index, offsets, atom, edge, gt, nt, tok.order_encoder.weight.detach(), Z, None, dims)
    o2, p2, m2 = torch.empty_like(out), torch.empty_like(idx), torch.empty_like(mask)
    grads = [torch.empty_like(t) for t in (atom, edge, gt, nt, tok.order_encoder.weight, Z)]
    nbytes = lib.me_graph_tokens_bwd_workspace(ctypes.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    s = _capi.stream_ptr

    def gemm():
        with torch.no_grad():
            tok._project(ids, Sn)

    def bwd(parts):
        _capi.check(lib.me_graph_tokens_bwd(ctypes.byref(d), dout.data_ptr(), *[g.data_ptr() for g in grads], 0, parts, ws.data_ptr(), nbytes, s()))
    return timed([gemm,
                  lambda: _capi.check(lib.me_graph_tokens_fwd(ctypes.byref(d), o2.data_ptr(), 0, p2.data_ptr(), m2.data_ptr(), s())),
                  lambda: bwd(_capi.ME_GRAPH_BWD_INDEX), lambda: bwd(_capi.ME_GRAPH_BWD_GATHER)], floor), nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rev", default=None, help="label of the measured tree for the header (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rev = args.rev
    if not rev:
        try:
            rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                 cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
        except OSError:
            rev = ""
    recipe = dict(num_atoms=512 * 9, num_edges=512 * 3, rand_node_id=False, orf_node_id=False, lap_node_id=True, lap_node_id_k=16,
                  lap_node_id_sign_flip=True, lap_node_id_eig_dropout=0.2, type_id=True, hidden_dim=768, n_layers=12)
    configs = {"recipe (lap 16)": recipe, "rand+orf 768, lap": dict(recipe, rand_node_id=True, rand_node_id_dim=768, orf_node_id=True,
                                                                    orf_node_id_dim=768)}
    lines = [f"# tools/graph_tokenizer_time.py --iters {args.iters} --rev {rev or 'unknown'!r}   ({torch.cuda.get_device_name(0)}; --rev names the tree)",
             f"# us per call: median (min-max) of 7 windows of >= {WINDOW_MS:.0f} ms, HIP and PyTorch windows alternating, 5 warm-up calls;",
             "# x = PyTorch median / HIP median; split = identifier GEMM with packing / assembly kernel / backward index build / backward gathers",
             f"{'config':<18} {'batch':<9} {'Sn':>5} {'Se':>5} {'T':>3} | {'fwd HIP':>22} {'fwd torch':>24} {'x':>5} | {'fwd+bwd HIP':>24} "
             f"{'fwd+bwd torch':>26} {'x':>5} | split (us)"]

    def cell(t):
        return f"{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})"
    for cname, cfg in configs.items():
        torch.manual_seed(0)
        tok = M.GraphFeatureTokenizer(**cfg).to(dev).eval()
        for bname, pile in (("molecules", False), ("pile-up", True)):
            bd = make_batch(dev, pile)
            Sn, Se = sum(bd["node_num"]), sum(bd["edge_num"])
            T = max(n + e for n, e in zip(bd["node_num"], bd["edge_num"]))
            with torch.no_grad():
                drawn = tok.node_identifiers(bd)
            node_ids = {k: v for k, v in drawn.items() if k != "lap"}
            ids = tok._identifiers(bd, bd["node_num"], node_ids)
            dout = torch.randn(len(bd["node_num"]), T + 2, 768, device=dev)
            params = list(tok.parameters())

            def hip_fwd():
                with torch.no_grad():
                    tok(bd, node_ids=node_ids)

            def pt_fwd():
                with torch.no_grad():
                    composition(tok, bd, ids)

            def hip_both():
                torch.autograd.grad(tok(bd, node_ids=node_ids)[0], params, dout)

            def pt_both():
                torch.autograd.grad(composition(tok, bd, ids)[0], params, dout)
            worst = float((tok(bd, node_ids=node_ids)[0] - composition(tok, bd, ids)[0]).abs().max())
            assert worst < 1e-4, worst
            f_hip, f_pt = timed([hip_fwd, pt_fwd], args.iters)
            b_hip, b_pt = timed([hip_both, pt_both], args.iters)
            parts, nbytes = split(tok, bd, ids, node_ids, args.iters)
            lines.append(f"{cname:<18} {bname:<9} {Sn:>5} {Se:>5} {T:>3} | {cell(f_hip):>22} {cell(f_pt):>24} {f_pt[0] / f_hip[0]:>5.2f} | "
                         f"{cell(b_hip):>24} {cell(b_pt):>26} {b_pt[0] / b_hip[0]:>5.2f} | "
                         + " / ".join(f"{p[0]:.1f}" for p in parts) + f"  (workspace {nbytes / 1e6:.1f} MB)")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
