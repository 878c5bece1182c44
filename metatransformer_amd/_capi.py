"""ctypes binding of libmetaenc.so (the C ABI declared in include/metaenc.h).

The north star asks for a "thin C-ABI cffi layer"; ``cffi`` is not installed in this image, so the same
C ABI is bound with the standard library's ``ctypes`` (no compile-time dependency, identical symbols).

The shared library is built in-tree (``python -m metatransformer_amd.build`` or ``__graft_entry__.build()``)
and MUST be present: there is no CPU or PyTorch fallback for any op -- loading fails loudly.

Nothing of the ABI is repeated here: the structure classes (``GemmDesc`` for ``me_gemm_desc``, ...), the ``ME_*`` constants and
``SIGNATURES`` are built at import from the header itself (``_header.py``).  A new entry point, field or constant is declared in
include/metaenc.h and nowhere else.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

import torch  # noqa: F401  (imported first so libamdhip64.so.7 resolves to the copy torch already loaded)

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmetaenc.so")


class MetaEncError(RuntimeError):
    pass


try:
    _CONSTANTS, _STRUCTS, _PROTOTYPES = _header.read()
except OSError as e:
    raise MetaEncError(f"the C ABI header was looked for at {_header.HEADER_PATH} and could not be read ({e}): the package "
                       "binds libmetaenc.so from include/metaenc.h of its source tree") from e

globals().update(_CONSTANTS)       # ME_F32, ME_GEMM_NT, ME_TC_BATCH, ...: every integer constant of the header

_SCALAR = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float, "size_t": c_size_t}
# structs that live in DEVICE memory: a pointer to one is passed as an address, like every other device pointer
_DEVICE_STRUCTS = ("me_adamw_segment", "me_adamw_ctl")


def _struct(pyname: str, cname: str, fields: list) -> type:
    def ctype(name, t):
        if isinstance(t, str):
            return _SCALAR.get(t, c_void_p)          # (the reader admits scalars and pointers only)
        members, count = t                           # struct { ... } name[count]
        return _struct(f"{pyname}_{name}", f"{cname}.{name}[]", members) * count
    return type(pyname, (ctypes.Structure,), {"_fields_": [(n, ctype(n, t)) for n, t in fields],
                                              "__doc__": f"``struct {cname}`` of include/metaenc.h"})


# C name -> class; each is also a module attribute under the CamelCase of its C name without me_ (me_attn_qkv_desc: AttnQkvDesc)
STRUCTS = {c: _struct("".join(w.capitalize() for w in c[3:].split("_")), c, f) for c, f in _STRUCTS.items()}
globals().update({cls.__name__: cls for cls in STRUCTS.values()})


def _argtype(t: str):
    if "*" not in t:
        return _SCALAR[t]
    target = t[:-1].replace("const ", "")
    if target in STRUCTS and target not in _DEVICE_STRUCTS:
        return POINTER(STRUCTS[target])
    return c_char_p if target == "char" else c_void_p


# name -> (restype, argtypes) of every prototype in the header
SIGNATURES = {name: (_argtype(ret), [_argtype(t) for t, _ in args]) for name, (ret, args) in _PROTOTYPES.items()}

_lib = None


def load() -> ctypes.CDLL:
    """Load libmetaenc.so and bind every declared symbol.  Raises MetaEncError if the library or a symbol is
    missing -- the product path never silently degrades to PyTorch ops."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise MetaEncError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m metatransformer_amd.build` "
            "(needs hipcc; cross-compiles gfx950 without a GPU). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise MetaEncError(f"libmetaenc.so does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    if lib.me_abi_version() != ME_ABI_VERSION:
        raise MetaEncError(f"libmetaenc.so ABI version {lib.me_abi_version()} != {ME_ABI_VERSION}; rebuild it")
    # profiling scripts switch the weight-gradient side stream off from outside (tools/prof_round.sh: kernels that share the chip
    # have no duration of their own).  The library reads no environment: the host does, and uses the ABI call.
    if os.environ.get("ME_WGRAD_OVERLAP", "1") == "0":
        lib.me_block_bwd_overlap(0)
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().me_last_error()
        raise MetaEncError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def dtype_code(dt: torch.dtype, storage: bool = False) -> int:
    if dt == torch.float32:
        return ME_F32
    if dt == torch.bfloat16:
        return ME_BF16
    if storage and dt == torch.float16:
        return ME_F16
    raise MetaEncError(f"unsupported dtype {dt}: libmetaenc computes in float32 or bfloat16"
                       + ("" if storage else " (float16 tensors are converted with ops.cast at the boundary)"))


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream
