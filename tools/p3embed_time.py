"""P3Embed timing at the recipe shapes: forward and forward + backward, split per stage and per kernel family.

    python tools/p3embed_time.py [--iters 5] [--json PATH]

Shapes: ScanObjectNN [32, 1024, 3] (bn, training mode, 1 stage) and S3DIS [8, 24000, 7] (ln2d, 2 stages), embed_dim 768.
Whole-call times are device events around the call after warm-up.  The per-stage and per-family split of the forward
brackets every library call with events in a separate (instrumented) pass; family = fps / knn / group (me_group_features) /
gemm (heads.linear) / norm+relu (LayerNorm2d or BatchNorm glue, ReLU) / pool / glue (the broadcast add of conv2's split
first layer and the remaining torch glue).  me_group_features_bwd is timed on its own per stage.
"""
import argparse
import json
import os
import sys
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metatransformer_amd as M  # noqa: E402
from metatransformer_amd import heads  # noqa: E402

CASES = {
    "scanobjectnn": (dict(sample_ratio=0.25, in_channels=3, norm_args="bn"), 32, 1024),
    "s3dis": (dict(sample_ratio=0.0625, in_channels=7, norm_args={"norm": "ln2d"}), 8, 24000),
}
COMMON = dict(group_size=32, layers=4, embed_dim=768, subsample="fps", group="knn", feature_type="dp_df", reduction="max")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


class Split:
    """event brackets around the library calls of one forward: ms per (stage, family)"""

    def __init__(self):
        self.ev, self.stage = [], 0

    def wrap(self, fam, fn):
        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.ev.append((self.stage, fam, e0, e1))
            return out
        return run

    def install(self, mp):
        for name, fam in (("furthest_point_sample", "fps"), ("knn_indices", "knn"), ("group_features", "group"),
                          ("linear", "gemm"), ("pool_tokens", "pool")):
            mp.append((heads, name, getattr(heads, name)))
            setattr(heads, name, self.wrap(fam, getattr(heads, name)))
        na = heads.P3Embed._norm_act
        mp.append((heads.P3Embed, "_norm_act", heads.P3Embed.__dict__["_norm_act"]))
        heads.P3Embed._norm_act = staticmethod(self.wrap("norm+relu", na))
        st = heads.P3Embed._stage
        split = self

        def stage(self_, *a):
            split.stage += 1
            return split.wrap("stage", lambda: st(self_, *a))()
        mp.append((heads.P3Embed, "_stage", st))
        heads.P3Embed._stage = stage

    def result(self):
        torch.cuda.synchronize()
        out = defaultdict(float)
        for s, fam, e0, e1 in self.ev:
            out[(s, fam)] += e0.elapsed_time(e1)
        res = {}
        for s in sorted({s for s, _ in out}):
            fams = {f: round(v, 3) for (ss, f), v in out.items() if ss == s and f != "stage"}
            fams["glue"] = round(out[(s, "stage")] - sum(fams.values()), 3)
            res[f"stage{s}"] = {"total_ms": round(out[(s, "stage")], 3), **fams}
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "p3embed_time needs a GPU"
    dev = torch.device("cuda:0")
    report = {}
    for name, (kw, B, N) in CASES.items():
        torch.manual_seed(0)
        mod = M.P3Embed(**COMMON, **kw).to(dev).train()
        p = (torch.rand(B, N, 3) * 2 - 1).to(dev)
        f = torch.randn(B, kw["in_channels"], N, device=dev)
        fr = f.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                mod(p, f)

        def fwd_bwd():
            _, out_f = mod(p, fr)
            sum(o.sum() for o in out_f[1:]).backward()
        r = {"shape": [B, N, kw["in_channels"]], "fwd_ms": round(timed(fwd, a.iters), 3),
             "fwd_bwd_ms": round(timed(fwd_bwd, a.iters), 3)}
        mp, split = [], Split()
        split.install(mp)
        try:
            fwd()
            r["fwd_split_ms"] = split.result()
        finally:
            for obj, nm, orig in reversed(mp):
                setattr(obj, nm, orig)
        # me_group_features_bwd per stage on the stage's own indices
        cur_p, cur_f, n = p, f.transpose(1, 2).contiguous(), N
        gb = {}
        for s, C in enumerate(mod.channel_list[:-1], start=1):
            n //= 4
            idx = heads.furthest_point_sample(cur_p, n)
            cp = torch.gather(cur_p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
            nbr = heads.knn_indices(cur_p, cp, 32)
            ff = cur_f.clone().requires_grad_(True)
            rows = heads.group_features(cur_p, ff, idx, nbr, "dp_df")
            go = torch.randn_like(rows)
            gb[f"stage{s}"] = round(timed(lambda: torch.autograd.grad(rows, ff, go, retain_graph=True), a.iters), 3)
            cur_p, cur_f = cp, torch.randn(B, n, mod.channel_list[s], device=dev)
        r["group_features_bwd_ms"] = gb
        r["peak_mem_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 1)
        report[name] = r
        print(json.dumps({name: r}), flush=True)
        del mod
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
