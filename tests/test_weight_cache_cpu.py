"""The Block weight-copy cache (metatransformer_amd/weight_cache.py) on the CPU: which copies each entry point builds, refreshes and
leaves alone, counted on plain-torch stand-ins for the library's cast / transpose / split ops -- and the one parameter order."""
import copy
import inspect

import pytest
import torch

from metatransformer_amd import Block, ops
from metatransformer_amd.encoder import _BlockFn
from metatransformer_amd.weight_cache import _WeightCache

NAMES = ("qkv", "proj", "fc1", "fc2")
KINDS = ("cast", "t", "x3", "x3t", "fold")
CPU = torch.device("cpu")


def planes(w, transposed):
    w = w.t() if transposed else w
    return torch.cat([w, w, w], dim=1).bfloat16()


@pytest.fixture
def calls(monkeypatch):
    """ops.* stand-ins; calls[name] lists the number of matrices of each call"""
    log = {n: [] for n in ("cast", "transpose_cast", "transpose_cast_many", "split3", "split3_many")}

    def one(name, fn):
        def f(x, *a, **k):
            log[name].append(1)
            return fn(x, *a, **k)
        monkeypatch.setattr(ops, name, f)

    def many(name, fn):
        def f(ws, arg, *a, **k):
            log[name].append(len(ws))
            return [fn(w, arg) for w in ws]
        monkeypatch.setattr(ops, name, f)
    one("cast", lambda x, dtype, out=None: x.to(dtype))
    one("transpose_cast", lambda w, dtype: w.t().contiguous().to(dtype))
    one("split3", lambda x, right_operand=False: planes(x, False))
    many("transpose_cast_many", lambda w, dtype: w.t().contiguous().to(dtype))
    many("split3_many", planes)
    return log


@pytest.fixture
def blocks():
    torch.manual_seed(0)
    bs = [Block(dim=8, num_heads=2) for _ in range(3)]
    for b in bs:
        b._wcache.bind(b)
    return bs


def weights(b):
    return {"qkv": b.attn.qkv.weight, "proj": b.attn.proj.weight, "fc1": b.mlp.fc1.weight, "fc2": b.mlp.fc2.weight}


def kinds_present(b):
    return {k for k in KINDS for n in NAMES if b._wcache.has(k, n, CPU)}


def test_transposed_builds_missing_and_refreshes_stale_copies_in_one_call(blocks, calls):
    b0, b1, b2 = blocks
    bf = torch.bfloat16
    tr = b0._wcache.transposed("qkv", b0.attn.qkv.weight, bf)
    assert calls["transpose_cast_many"] == [12]                   # cold: all 12 copies, the other blocks' missing ones included
    assert torch.equal(tr, b0.attn.qkv.weight.detach().t().to(bf))
    assert all(b._wcache.has("t", n, CPU) for b in blocks for n in NAMES) and all(kinds_present(b) == {"t"} for b in blocks)
    for b in blocks:
        for n, w in weights(b).items():
            assert torch.equal(b._wcache.transposed(n, w, bf), w.detach().t().to(bf))
    assert calls["transpose_cast_many"] == [12]                   # all fresh: no call
    with torch.no_grad():
        b1.mlp.fc1.weight.mul_(2)                                 # one weight moves (its version does)
    b0._wcache.transposed("qkv", b0.attn.qkv.weight, bf)          # (a fresh copy is handed out without a scan)
    assert calls["transpose_cast_many"] == [12]
    tr = b1._wcache.transposed("fc1", b1.mlp.fc1.weight, bf)
    assert calls["transpose_cast_many"] == [12, 1]                # exactly the stale one
    assert torch.equal(tr, b1.mlp.fc1.weight.detach().t().to(bf))
    ops.weights_updated()                                         # the fused optimizer's epoch: parameters outside a FlatParams keep their copies
    for b in blocks:
        for n, w in weights(b).items():
            b._wcache.transposed(n, w, bf)
    assert calls["transpose_cast_many"] == [12, 1]
    b2.attn.proj.weight._me_flat = object()                       # (one that claims to live in a FlatParams follows the epoch)
    b2._wcache.transposed("proj", b2.attn.proj.weight, bf)        # its key now carries the epoch
    ops.weights_updated()
    b2._wcache.transposed("proj", b2.attn.proj.weight, bf)
    assert calls["transpose_cast_many"] == [12, 1, 1, 1]
    assert _WeightCache.prefetch_transposed(CPU) == 0 and calls["transpose_cast_many"] == [12, 1, 1, 1]      # nothing stale
    assert not any(calls[n] for n in ("cast", "transpose_cast", "split3", "split3_many"))


def test_split3_refreshes_stale_copies_but_creates_none(blocks, calls):
    b0, b1, b2 = blocks
    for b in (b0, b1):
        x3 = b._wcache.split3("qkv", b.attn.qkv.weight, False)
        assert torch.equal(x3, planes(b.attn.qkv.weight.detach(), False))
    assert calls["split3_many"] == [1, 1]                         # each its own: the others' copies are missing, not stale
    with torch.no_grad():
        b0.attn.qkv.weight.mul_(2)
    x3 = b1._wcache.split3("proj", b1.attn.proj.weight, False)
    assert calls["split3_many"] == [1, 1, 2]                      # the caller's missing copy + block 0's stale one
    assert torch.equal(x3, planes(b1.attn.proj.weight.detach(), False))
    assert torch.equal(b0._wcache.split3("qkv", b0.attn.qkv.weight, False), planes(b0.attn.qkv.weight.detach(), False))
    assert calls["split3_many"] == [1, 1, 2]                      # (refreshed by block 1's call)
    present = {(i, k, n) for i, b in enumerate(blocks) for k in KINDS for n in NAMES if b._wcache.has(k, n, CPU)}
    assert present == {(0, "x3", "qkv"), (1, "x3", "qkv"), (1, "x3", "proj")}
    x3t = b2._wcache.split3("fc2", b2.mlp.fc2.weight, True)       # the transposed kind is a table of its own
    assert calls["split3_many"] == [1, 1, 2, 1] and torch.equal(x3t, planes(b2.mlp.fc2.weight.detach(), True))
    assert not calls["transpose_cast_many"]
    b0._wcache.transposed("qkv", b0.attn.qkv.weight, torch.bfloat16)      # whereas transposed() does create the missing ones
    assert calls["transpose_cast_many"] == [12] and all(b._wcache.has("t", n, CPU) for b in blocks for n in NAMES)


def test_copies_do_not_follow_a_deepcopy(blocks, calls):
    b0 = blocks[0]
    b0._wcache.operands(weights(b0), torch.bfloat16, False, True)
    b0._wcache.operands(weights(b0), torch.float32, True, True)
    assert kinds_present(b0) == {"cast", "t", "x3", "x3t"}
    assert kinds_present(copy.deepcopy(b0)) == set()


def test_operands_builds_the_copies_of_its_compute_mode_only(blocks, calls):
    b0, b1, _ = blocks
    w, wt = b0._wcache.operands(weights(b0), torch.float32, True, True)
    assert kinds_present(b0) == {"x3", "x3t"}
    for n, p in weights(b0).items():
        assert torch.equal(w[n], planes(p.detach(), False)) and torch.equal(wt[n], planes(p.detach(), True))
    w, wt = b1._wcache.operands(weights(b1), torch.bfloat16, False, True)
    assert kinds_present(b1) == {"cast", "t"}
    for n, p in weights(b1).items():
        assert torch.equal(w[n], p.detach().bfloat16()) and torch.equal(wt[n], p.detach().t().bfloat16())
    w, wt = b1._wcache.operands(weights(b1), torch.bfloat16, False, False)
    assert wt is None and set(w) == set(NAMES)


def test_block_params_order_is_the_autograd_function_s():
    names = list(inspect.signature(_BlockFn.forward).parameters)
    assert names[:2] == ["ctx", "x"]
    fields = Block(dim=8, num_heads=2)._params()._fields
    assert list(fields) == names[2:2 + len(fields)] and len(fields) == 14 and fields[-2:] == ("gamma1", "gamma2")
