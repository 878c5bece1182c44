"""Compute copies of the four weight matrices of a Block (qkv, proj, fc1, fc2), rebuilt when the parameter changes."""
from typing import Optional
import weakref

import torch

from . import ops


def _tensor_version(t: torch.Tensor):
    """``t._version``, or None for inference tensors (``torch.inference_mode()``: no version counter, reading the attribute raises)."""
    try:
        return t._version
    except RuntimeError:
        return None


class _WeightCache:
    """One table per Block: slot (kind, name, device) -> (key, copy); a copy is rebuilt when its key, the parameter's identity and
    version, has moved (optimizer step / load_state_dict / .to()).  nn.DataParallel replicas share this object: hence the device.
        cast  [out, in] in the compute dtype       t    [in, out] in the compute dtype            (forward / dgrad GEMMs)
        x3    ME_BF16X3 planes of W, [out, 3 in]   x3t  of W^T, [in, 3 out]                       (the same, fp32_mode = "3xbf16")
        fold  (W', s, c) of a Linear with the LayerNorm before it folded in                       (folded inference)
    `cast` and `fold` copies are rebuilt one at a time (bf16 `cast` copies come straight out of the fused optimizer's bf16 mirror
    when the parameters live in a parallel.FlatParams).  A missing or stale `t` / `x3` / `x3t` copy triggers ONE batched launch that
    also refreshes the copies of its kind of every live Block on the device (`_scan` finds them, `_refresh` rebuilds them): after
    an optimizer step that is all of them, one launch instead of four per block."""
    _live = weakref.WeakSet()      # all caches
    _pending = {}         # device -> event behind a refresh of the transposed copies that ran on another stream (prefetch_transposed)

    def __init__(self):
        self._table = {}
        self._owner = lambda: None          # weakref to the Block (bind)
        _WeightCache._live.add(self)

    # a cache is derived state: copies / pickles of a Block start with an empty one (re-bound to the new owner on first use)
    def __deepcopy__(self, memo):
        return _WeightCache()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()

    def bind(self, blk) -> None:
        if self._owner() is not blk:
            self._owner = weakref.ref(blk)

    def has(self, kind: str, name: str, device) -> bool:
        return (kind, name, device) in self._table

    def weights(self):      # the owner's four matrices under the names their copies go by
        blk = self._owner()
        return {} if blk is None else {"qkv": blk.attn.qkv.weight, "proj": blk.attn.proj.weight, "fc1": blk.mlp.fc1.weight, "fc2": blk.mlp.fc2.weight}

    @staticmethod
    def _key(p: torch.Tensor, dtype):
        # (dtype: the copy's target dtype, None for the kinds that have only one)  WEIGHT_EPOCH covers the fused optimizer, which writes
        # parameters through raw pointers (no _version bump); it only ever touches parameters that live in a parallel.FlatParams, so
        # other (e.g. frozen) encoders keep their copies
        epoch = ops.WEIGHT_EPOCH if hasattr(p, "_me_flat") else 0
        return (p.data_ptr(), _tensor_version(p), epoch, p.dtype, p.device, dtype)

    @classmethod
    def _scan(cls, kind: str, device, *, missing: bool, dtype=None, src_dtype=None, contiguous: bool = False):
        """(cache, name, key, weight) of every 2-D weight of every live Block on `device` whose `kind` copy is stale -- or, with
        `missing`, does not exist yet.  dtype: the target dtype the copies must have (None, without `missing` only: the one each existing copy has);
        src_dtype: only parameters of this dtype; contiguous: only contiguous parameters."""
        todo = []
        for c in list(cls._live):
            for n, w in c.weights().items():
                if w.device != device or w.dim() != 2 or src_dtype not in (None, w.dtype) or (contiguous and not w.is_contiguous()):
                    continue
                h = c._table.get((kind, n, w.device))
                if h is not None or missing:
                    k = cls._key(w, h[0][-1] if dtype is None else dtype)
                    if h is None or h[0] != k:
                        todo.append((c, n, k, w))
        return todo

    @staticmethod
    def _refresh(kind: str, todo, mine=None):
        """Rebuild the `kind` copy of every (cache, name, key, weight) of `todo` with the batched op of the kind -- one call per
        (source dtype, target dtype) -- and write the results back.  Returns the copy of the entry `mine`, from a local: the table
        is shared with the threads of other DataParallel replicas, which may rewrite the slot at any time."""
        groups = {}
        for e in todo:
            groups.setdefault((e[3].dtype, e[2][-1]), []).append(e)
        own = None
        for (_, dtype), entries in groups.items():
            ws = [w.detach().contiguous() for _, _, _, w in entries]
            outs = ops.transpose_cast_many(ws, dtype) if kind == "t" else ops.split3_many(ws, kind == "x3t")
            for e, t in zip(entries, outs):
                c, n, k, w = e
                c._table[(kind, n, w.device)] = (k, t)
                if e is mine:
                    own = t
        return own

    def fwd(self, name: str, p: torch.Tensor, dtype) -> torch.Tensor:
        if p.dtype == dtype:
            return p.detach()
        if dtype == torch.bfloat16:
            flat = getattr(p, "_me_flat", None)
            if flat is not None:
                v = flat.bf16_view(p)
                if v is not None:
                    return v
        k = self._key(p, dtype)
        slot = ("cast", name, p.device)
        hit = self._table.get(slot)
        if hit is None or hit[0] != k:
            hit = (k, ops.cast(p.detach().contiguous(), dtype))
            self._table[slot] = hit
        return hit[1]

    def transposed(self, name: str, p: torch.Tensor, dtype) -> torch.Tensor:
        k = self._key(p, dtype)
        ev = _WeightCache._pending.pop(p.device, None)
        if ev is not None:                      # copies rebuilt on the optimizer's side stream (prefetch_transposed): order this stream behind it
            torch.cuda.current_stream(p.device).wait_event(ev)
        hit = self._table.get(("t", name, p.device))
        if hit is not None and hit[0] == k:
            return hit[1]
        # with this one, every copy on the device that is stale or was never built, for the parameters of this one's dtype
        todo = self._scan("t", p.device, missing=True, dtype=dtype, src_dtype=p.dtype)
        mine = next((e for e in todo if e[0] is self and e[1] == name and e[2] == k), None)
        if mine is None:                        # (a DataParallel replica: its parameters are not the owner's)
            mine = (self, name, k, p)
            todo.append(mine)
        return self._refresh("t", todo, mine)

    def split3(self, name: str, p: torch.Tensor, transposed: bool) -> torch.Tensor:
        """ME_BF16X3 right-operand copy of a weight ([out, 3 in]; transposed: of W^T, [in, 3 out] for the dgrad GEMMs): the
        fp32-accurate mode's compute copies."""
        kind = "x3t" if transposed else "x3"
        k = self._key(p, None)
        slot = (kind, name, p.device)
        hit = self._table.get(slot)
        if hit is not None and hit[0] == k:
            return hit[1]
        if p.dtype != torch.float32 or not p.is_contiguous():
            w32 = ops.cast(p.detach().contiguous(), torch.float32)
            w32 = ops.transpose_cast(w32, torch.float32) if transposed else w32
            out = ops.split3(w32, right_operand=True)
            self._table[slot] = (k, out)
            return out
        # with this one, every STALE copy of the kind on the device, never a missing one (a block that does not run in this mode gets none)
        mine = (self, name, k, p)
        todo = [mine] + [e for e in self._scan(kind, p.device, missing=False, src_dtype=torch.float32, contiguous=True)
                         if not (e[0] is self and e[1] == name)]
        return self._refresh(kind, todo, mine)

    @classmethod
    def prefetch_transposed(cls, device) -> int:
        """Rebuild, on the CURRENT stream, every transposed copy that exists on `device` and is stale (one batched launch per
        dtype) -- FusedAdamW(overlap=True) calls this on its side stream right behind an optimizer step, so that the 0.15 ms of weight
        transposes run under the next forward instead of at the head of the next backward.  The first `transposed()` hit afterwards
        makes its stream wait for the event recorded here.  Returns the number of copies rebuilt."""
        todo = cls._scan("t", device, missing=False)
        cls._refresh("t", todo)
        if todo:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            cls._pending[device] = ev
        return len(todo)

    def operands(self, weights, cdt, x3: bool, transposed: bool):
        """(w, wt): name -> the right operand the forward GEMMs of a compute mode read and, with `transposed`, the one its dgrad GEMMs
        read (else wt is None).  weights: name -> parameter.  x3: the fp32-accurate three-product mode; else compute dtype `cdt`."""
        w, wt = {}, ({} if transposed else None)
        for k, p in weights.items():
            w[k] = self.split3(k, p, False) if x3 else self.fwd(k, p, cdt)
            if transposed:
                wt[k] = self.split3(k, p, True) if x3 else self.transposed(k, p, cdt)
        return w, wt

    def folded(self, name: str, w: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, bias: Optional[torch.Tensor], dtype):
        """LayerNorm folded into the Linear behind it (inference; me_gemm_desc.row_affine):
            Linear(LN(x))[m, n] = rstd_m (x W'^T)[m, n] - rstd_m mean_m s[n] + c[n]
        with W' = gamma o W rounded to the compute dtype, s[n] = sum_k W'[n, k] of the ROUNDED values (so that the mean
        component cancels exactly as the kernel sees it) and c = W beta + bias from the fp32 masters.  One-off weight
        preparation in torch (plumbing), cached like the other compute copies."""
        k = tuple(self._key(t, dtype) for t in (w, ln_w, ln_b) + ((bias,) if bias is not None else ()))
        slot = ("fold", name, w.device)
        hit = self._table.get(slot)
        if hit is None or hit[0] != k:
            with torch.no_grad():
                # every number here comes out of the library (this used to be at::native mul / reduce kernels):
                #   W' = gamma o W rounded to the compute dtype   -- the column-scale form of me_dropout_add (p = 0)
                #   s  = W' 1   (of the ROUNDED values, fp32 sums) -- me_gemm: four rows of ones x W'^T, row 0
                #   c  = W beta + bias                             -- exact-fp32 me_gemm: four copies of beta x W^T + the bias epilogue
                w32 = ops.cast(w.detach().contiguous(), torch.float32)
                g32, b32 = ops._f32(ln_w.detach()).contiguous(), ops._f32(ln_b.detach()).contiguous()
                wf = ops.dropout_add(w32, None, w32.shape[0], 0.0, 0.0, 0, out_dtype=dtype, colscale=g32)
                K = w32.shape[1]
                ones = torch.ones((4, K), dtype=dtype, device=w.device)
                s_vec = ops.gemm(ones, wf, out_dtype=torch.float32)[0].contiguous()
                c_vec = ops.gemm(b32[None, :].expand(4, K).contiguous(), w32, bias=None if bias is None else ops._f32(bias.detach()),
                                 out_dtype=torch.float32)[0].contiguous()
                hit = (k, (wf, s_vec, c_vec))
            self._table[slot] = hit
        return hit[1]
