"""CPU: the drop-in boundary -- the C-ABI library loads and exports every symbol include/metaenc.h declares; what the ctypes binding
derives from the header (struct layouts, prototypes, constants) is what gcc sees in it; the product package never touches oracle/, and the
host-side module mirrors the reference's plugin interface (names, shapes, error behaviour)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch
import torch.nn as nn

from conftest import ROOT

import metatransformer_amd as M
from metatransformer_amd import _capi, _header, build as me_build
from oracle import block_oracle as bo

HEADER = os.path.join(ROOT, "include", "metaenc.h")


@pytest.fixture(scope="module")
def lib():
    me_build.build(verbose=False)
    return _capi.load()


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_all_bound_and_exported(lib):
    names = header_functions()
    assert len(names) >= 18
    assert set(names) == set(_capi.SIGNATURES), "include/metaenc.h and _capi.SIGNATURES disagree"
    for n in names:
        assert hasattr(lib, n), f"libmetaenc.so does not export {n}"
    assert lib.me_abi_version() == 1
    assert lib.me_build_arch() == b"gfx950"


def run_c(code, run=True):
    """compile `code` (which includes metaenc.h) with gcc -Werror; run=True: -> {first word: second word} of the lines it prints"""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "metaenc.h"\n' + code)
        gcc = ["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), src]
        res = subprocess.run(gcc + (["-o", exe] if run else ["-fsyntax-only"]), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        if run:
            return dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if l)


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_every_struct_body_of_the_header_is_mirrored():
    assert set(re.findall(r"typedef\s+struct\s+(me_\w+)\s*\{", header_text())) == set(_capi.STRUCTS) == set(_header.read()[1])
    for cname, cls in _capi.STRUCTS.items():
        assert getattr(_capi, cls.__name__) is cls and cls.__name__ == "".join(w.capitalize() for w in cname[3:].split("_"))
    assert {"GemmDesc", "AttnQkvDesc", "TcBatch", "GemmProfileRec"} <= {c.__name__ for c in _capi.STRUCTS.values()}


@pytest.mark.parametrize("cname,pyname", [(c, cls.__name__) for c, cls in _capi.STRUCTS.items()])
def test_struct_layouts_match_c(cname, pyname):
    """every struct that crosses the C ABI: size and field offsets of the ctypes class == what gcc lays out from the header; of an
    array of nested structs the members of elements 0 and 1"""
    cls = getattr(_capi, pyname)
    want = {}
    for name, ft in cls._fields_:
        want[name] = getattr(cls, name).offset
        if hasattr(ft, "_length_"):
            assert ft._length_ >= 2
            for i in (0, 1):
                for sub, _ in ft._type_._fields_:
                    want[f"{name}[{i}].{sub}"] = want[name] + i * ctypes.sizeof(ft._type_) + getattr(ft._type_, sub).offset
    assert [n for n, _ in cls._fields_] == [n for n, _ in _header.read()[1][cname]]
    got = run_c(f'int main(void){{ printf("size %zu\\n", sizeof({cname}));\n'
                + "".join(f'printf("{f} %zu\\n", offsetof({cname}, {f}));\n' for f in want) + "return 0; }\n")
    assert int(got.pop("size")) == ctypes.sizeof(cls)
    assert {k: int(v) for k, v in got.items()} == want


def test_parsed_prototypes_redeclare_without_conflict():
    """the compiler checks the reader: every function re-declared from the PARSED types behind the header's own declaration -- a type
    read wrongly, an argument lost or added is a conflicting redeclaration, a compile error"""
    protos = _header.read()[2]
    assert sorted(protos) == header_functions() and len(protos) >= 107
    run_c("".join(f"{ret} {name}({', '.join(f'{t} a{i}' for i, (t, _) in enumerate(args)) or 'void'});\n"
                  for name, (ret, args) in protos.items()), run=False)
    with pytest.raises(AssertionError, match="conflicting types"):          # (the check does fail on a wrong type)
        run_c("int me_cast(const void* a0, int a1, void* a2, int a3, int a4, void* a5);\n", run=False)


def test_c_types_map_to_ctypes():
    """the C-to-ctypes table, pinned by argument lists written out by hand"""
    from ctypes import POINTER, c_char_p, c_float as F, c_int as I, c_int64 as L, c_size_t, c_uint64, c_void_p as P
    S = _capi.SIGNATURES
    assert S["me_mae_loss"] == (I, [P, I] + [I] * 8 + [P, P, P, P, I, P, I, L, I, P, P, P, P, L, P, L, P])
    assert S["me_attention_bwd"] == (I, [P, L, P, L, P, L, P, P, P, L, I, I, I, I, F, I, F, c_uint64, P])
    assert S["me_dropout_add"] == (I, [P, I, P, I, P, I, L, I, L, F, F, c_uint64, P, P])
    assert S["me_device_info"] == (I, [I, P, P, P, c_char_p, I])
    assert S["me_block_fwd"] == (I, [POINTER(_capi.BlockDesc), P, P, P, P, c_size_t, P])
    assert S["me_block_bwd"][1][5] is POINTER(_capi.BlockGrads) and S["me_gemm_profile_read"][1] == [POINTER(_capi.GemmProfileRec), I]
    assert S["me_last_error"] == (c_char_p, []) and S["me_block_saved_bytes"] == (c_size_t, [POINTER(_capi.BlockDesc)])
    # the AdamW control block and segment table live in device memory: addresses, like every other device pointer
    assert S["me_adamw_prepare"][1][0] is P and S["me_adamw_step_segments"][1][5] is P and S["me_adamw_step_segments"][1][11] is P
    assert [t for _, t in _capi.AttnQkvDesc._fields_][:4] == [P, P, P, L] and dict(_capi.AttnQkvDesc._fields_)["seed"] is c_uint64
    assert dict(_capi.GemmDesc._fields_)["alpha"] is F and dict(_capi.GemmDesc._fields_)["op"] is ctypes.c_int32


def test_constants_equal_what_the_compiler_sees():
    consts = _header.read()[0]
    names = set(re.findall(r"\b(ME_[A-Z0-9_]+)\s*=", header_text())) | set(re.findall(r"#define\s+(ME_\w+)[ \t]+\S", header_text()))
    assert set(consts) == names and len(names) >= 47
    got = run_c("int main(void){\n" + "".join(f'printf("{n} %lld\\n", (long long){n});\n' for n in consts) + "return 0; }\n")
    assert {k: int(v) for k, v in got.items()} == consts == {n: getattr(_capi, n) for n in consts}
    # values that callers and stored records rely on
    pinned = dict(ME_ABI_VERSION=1, ME_F32=0, ME_BF16=1, ME_F16=2, ME_GROUP_DP=0, ME_GROUP_DP_FJ=1, ME_GROUP_DP_DF=2, ME_GROUP_DP_FJ_DF=3,
                  ME_GRAPH_BWD_INDEX=1, ME_GRAPH_BWD_GATHER=2, ME_ERR_UNSUPPORTED=-2)
    assert {n: consts[n] for n in pinned} == pinned
    from metatransformer_amd import audio
    assert audio.FRAMES_PER_WORKGROUP == consts["ME_FBANK_RUN"]


@pytest.mark.parametrize("text,word", [
    ("int me_x(int a, double b);", "double"),                                        # a scalar outside the table
    ("int me_x(int a, int);", "argument 'int'"),                                               # an argument without a name
    ("typedef struct me_s { int32_t a; long b; } me_s;", "long"),
    ("typedef struct me_s { int32_t a[4]; } me_s;", "a[4]"),                          # arrays only of nested structs
    ("typedef struct me_s { struct { struct { int a; } x[2]; } y[2]; } me_s;", "nested"),
    ("typedef struct me_s { struct { int a; } x[ME_NOWHERE]; } me_s;", "ME_NOWHERE"),
    ("typedef struct me_s { int a; } me_t;", "me_s"),
    ("enum { ME_A = 0, ME_B };", "ME_B"),
    ("enum { ME_A = 1 << 2 };", "ME_A"),
    ("#define ME_Z 1.5\n", "ME_Z"),
    ("union me_u { int a; float b; };", "me_u"),
    ("int me_x(int a)", "me_x"),                                                     # no semicolon
    ("int me_x(int (*cb)(int));", "me_x"),
])
def test_reader_raises_on_what_it_does_not_understand(text, word):
    with pytest.raises(_header.HeaderError, match=re.escape(word)):
        _header.parse("int me_ok(void);\n" + text)


def test_reader_reads_the_forms_the_header_uses():
    c, s, p = _header.parse("""#ifndef X_H
        #define X_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define ME_N 3   /* three */
        enum { ME_A = 0, ME_B = -2 /* , ME_C = 5 */ };
        typedef struct me_opaque me_opaque;
        typedef struct me_s { const void *p, *q; int64_t M, N; float* f; struct { void* src; int64_t rows, cols; } item[ME_N]; size_t n; } me_s;
        const char* me_name(void);
        size_t me_f(const me_s* d, me_opaque** h, const float* const* tables, uint64_t seed /* seed */, void* stream);
        #ifdef __cplusplus
        }
        #endif
        #endif""")
    assert c == dict(ME_N=3, ME_A=0, ME_B=-2)
    assert s == {"me_s": [("p", "const void*"), ("q", "const void*"), ("M", "int64_t"), ("N", "int64_t"), ("f", "float*"),
                          ("item", ([("src", "void*"), ("rows", "int64_t"), ("cols", "int64_t")], 3)), ("n", "size_t")]}
    assert p == {"me_name": ("const char*", []),
                 "me_f": ("size_t", [("const me_s*", "d"), ("me_opaque**", "h"), ("const float* const*", "tables"), ("uint64_t", "seed"),
                                     ("void*", "stream")])}


def test_missing_header_fails_loudly(monkeypatch):
    import importlib.util
    monkeypatch.setattr(_header, "HEADER_PATH", "/nonexistent/include/metaenc.h")
    spec = importlib.util.spec_from_file_location("metatransformer_amd._capi_without_header", _capi.__file__)
    with pytest.raises(RuntimeError, match="looked for at /nonexistent/include/metaenc.h") as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "MetaEncError"


def test_patch_embed_fuses_the_reference_geometries(lib):
    """host-side decision only (no kernel runs): the image and tubelet embeds of the reference gather inside the GEMM's operand stager
    when pixels and weight are bf16 -- since round 6 the spectrogram's stride-10 patches too (patch rows only have to be dword-aligned);
    fp32 arithmetic, odd patch shapes and odd image widths take the two-pass route and ask for a workspace"""
    def desc(shape, geom, xdt=_capi.ME_BF16, wdt=_capi.ME_BF16, cout=768):
        d = _capi.PatchEmbedDesc()
        d.x, d.x_dtype = 4096, xdt                                  # (an aligned address; never dereferenced by these two queries)
        B, Cin, T, H, W = shape
        d.B, d.Cin, d.T, d.H, d.W = B, Cin, T, H, W
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw = geom
        d.w_dtype, d.Cout = wdt, cout
        return d
    image = desc((256, 3, 1, 224, 224), (1, 16, 16, 1, 16, 16))                      # Data2Seq/Image.py:19-28
    video = desc((8, 3, 16, 224, 224), (2, 16, 16, 2, 16, 16))                       # Video/models/modeling_finetune.py:283-297
    audio = desc((12, 1, 1, 128, 1024), (1, 16, 16, 1, 10, 10))                      # Audio/src/models/ast_models.py:86
    for d, want in ((image, 1), (video, 1), (audio, 1), (desc((2, 3, 1, 224, 224), (1, 16, 16, 1, 16, 16), xdt=_capi.ME_F32), 0),
                    (desc((2, 3, 1, 224, 224), (1, 16, 16, 1, 16, 16), xdt=_capi.ME_F32, wdt=_capi.ME_F32), 0),
                    (desc((2, 3, 1, 224, 224), (1, 14, 14, 1, 14, 14)), 0), (desc((2, 3, 1, 220, 220), (1, 16, 16, 1, 16, 16)), 1),
                    (desc((2, 3, 1, 224, 221), (1, 16, 16, 1, 16, 16)), 0), (desc((2, 1, 1, 128, 100), (1, 16, 16, 1, 10, 9)), 0),
                    (desc((2, 3, 1, 224, 224), (1, 16, 16, 1, 16, 16), cout=772), 0)):
        assert lib.me_patch_embed_fused(ctypes.byref(d)) == want
        assert (lib.me_patch_embed_workspace_bytes(ctypes.byref(d)) == 0) == bool(want)
    bad = desc((2, 3, 1, 8, 8), (1, 16, 16, 1, 16, 16))
    assert lib.me_patch_embed_fused(ctypes.byref(bad)) == 0 and lib.me_patch_embed(ctypes.byref(bad), None) != 0
    assert b"kernel larger than input" in lib.me_last_error()


def test_gemm_planning_queries_of_round_6(lib):
    """host-side decisions only (no kernel runs): me_gemm_takes_row_parts (LayerNorm partials consumed by the folded GEMM), me_gemm_takes_a_wrap
    (A as two planes with a wrapped reduction), and the workspace query under me_gemm_reserve_cus (weight gradients on fewer workgroups: the query
    must cover either plan)"""
    def desc(M_, N_, K_, op=_capi.ME_GEMM_NT, cdt=_capi.ME_BF16, lda=None, ldb=None):
        d = _capi.GemmDesc()
        d.op, d.ab_dtype, d.M, d.N, d.K = op, _capi.ME_BF16, M_, N_, K_
        d.A, d.lda = 4096, lda or (K_ if op == _capi.ME_GEMM_NT else M_)
        d.B, d.ldb = 8192, ldb or (K_ if op == _capi.ME_GEMM_NT else N_)
        d.C, d.ldc, d.c_dtype, d.alpha = 16384, N_, cdt, 1.0
        return d
    # row_parts: K = 256 .. 1024 in steps of 256, every CU a 256 x 256 tile, bf16 output, plain bias / GELU epilogue
    for M_, N_, K_, want in ((50432, 2304, 768, 1), (50432, 3072, 768, 1), (65536, 4096, 1024, 1), (4096, 2304, 768, 0), (50432, 2304, 384, 0),
                             (50432, 2304, 1280, 0)):
        d = desc(M_, N_, K_)
        d.col_shift, d.row_parts, d.row_nparts, d.row_eps = 32768, 65536, max(K_ // 256, 1), 1e-6
        assert lib.me_gemm_takes_row_parts(ctypes.byref(d)) == want, (M_, N_, K_)
    d = desc(50432, 2304, 768, cdt=_capi.ME_F32)
    d.col_shift, d.row_parts, d.row_nparts, d.row_eps = 32768, 65536, 3, 1e-6
    assert lib.me_gemm_takes_row_parts(ctypes.byref(d)) == 0              # (the resident kernel writes bf16)
    # a_wrap_k: the one-tile 256 x 256 family, plain or fp32-residual epilogue
    for M_, N_, Kc, want in ((50432, 768, 3072, 1), (8192, 1024, 4096, 1), (512, 768, 3072, 0)):
        d = desc(M_, N_, 3 * Kc, cdt=_capi.ME_F32, lda=2 * Kc)
        d.a_wrap_k = 2 * Kc
        assert lib.me_gemm_takes_a_wrap(ctypes.byref(d)) == want, (M_, N_, Kc)
    d = desc(50432, 768, 9216, cdt=_capi.ME_F32, lda=6144)
    d.a_wrap_k = 6144 + 64                                                 # not a multiple of 128
    assert lib.me_gemm_takes_a_wrap(ctypes.byref(d)) == 0
    d.a_wrap_k, d.act, d.colscale = 6144, _capi.ME_ACT_GELU, 32768          # GELU next to a column scale: no (GELU alone is no either)
    assert lib.me_gemm_takes_a_wrap(ctypes.byref(d)) == 0
    d.act = _capi.ME_ACT_NONE
    assert lib.me_gemm_takes_a_wrap(ctypes.byref(d)) == 1
    # weight gradients: the workspace query with a reservation covers the default plan too (more slabs per tile, never fewer bytes)
    for Mo, No in ((2304, 768), (768, 3072), (768, 768)):
        d = desc(Mo, No, 50432, op=_capi.ME_GEMM_TN, cdt=_capi.ME_F32)
        w0 = lib.me_gemm_workspace_bytes(ctypes.byref(d))
        prev = lib.me_gemm_reserve_cus(16)
        try:
            w16 = lib.me_gemm_workspace_bytes(ctypes.byref(d))
        finally:
            assert lib.me_gemm_reserve_cus(prev) == 16
        assert w0 > 0 and w16 >= w0, (Mo, No, w0, w16)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "metatransformer_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "oracle/_ref" not in txt and "/root/reference" not in txt, f


def test_no_cpu_fallback():
    enc = M.build_encoder(1, 64, 2)
    with pytest.raises(M.MetaEncError, match="no CPU fallback"):
        enc(torch.randn(1, 3, 64))
    with pytest.raises(M.MetaEncError):
        M.PatchEmbed(img_size=32, embed_dim=64)(torch.randn(1, 3, 32, 32))
    with pytest.raises(M.MetaEncError):
        M.DataEmbedding(c_in=3, d_model=64).eval()(torch.randn(1, 8, 3))


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libmetaenc.so")
    with pytest.raises(M.MetaEncError, match="not built"):
        _capi.load()


def test_block_mirrors_reference_interface():
    # README.md:125-135 construction, verbatim keyword set
    enc = nn.Sequential(*[M.Block(dim=64, num_heads=4, mlp_ratio=4., qkv_bias=True, norm_layer=nn.LayerNorm,
                                  act_layer=nn.GELU) for _ in range(3)])
    sd = bo.make_encoder_state_dict(3, 64, seed=0)
    assert list(enc.state_dict().keys()) == list(sd.keys())
    assert all(enc.state_dict()[k].shape == v.shape for k, v in sd.items())
    enc.load_state_dict(sd, strict=True)
    # strict=True must reject a foreign key set, like the reference call sites rely on
    bad = dict(sd); bad["0.attn.q_bias"] = torch.zeros(64)
    with pytest.raises(RuntimeError):
        enc.load_state_dict(bad, strict=True)
    # indexable / sliceable / iterable (vit_adapter.py:107, X-Ray/train.py:80)
    assert isinstance(enc[1], M.Block) and len(enc[0:2]) == 2 and len(list(enc)) == 3
    # freezing + optimizer grouping by name (Video/optim_factory.py:30-41,67-73)
    for p in enc.parameters():
        p.requires_grad = False
    assert not any(p.requires_grad for p in enc.parameters())
    names = [n for n, _ in enc.named_parameters()]
    assert "1.mlp.fc1.bias" in names and all(len(p.shape) == 1 or n.endswith(".weight") for n, p in enc.named_parameters())
    # eps routes: default 1e-5, timm-factory sites 1e-6 via partial
    from functools import partial
    assert M.Block(64, 4).eps == 1e-5
    assert M.Block(64, 4, norm_layer=partial(nn.LayerNorm, eps=1e-6)).eps == 1e-6
    assert M.Block(768, 32).attn.scale == 24 ** -0.5          # Graph call site: 32 heads, head_dim 24
    with pytest.raises(M.MetaEncError):
        M.Block(64, 5)


def test_set_fp32_mode_reaches_every_block_of_a_task_model():
    """one line at an fp32 call site selects the fp32-accurate three-product arithmetic for the whole encoder, wherever it sits"""
    import torch
    enc = M.build_encoder(3, 256, 4)
    model = torch.nn.ModuleDict({"tokenizer": torch.nn.Linear(7, 256), "encoder": enc, "head": torch.nn.Linear(256, 10)})
    assert all(b.fp32_mode == "3xbf16" for b in enc)              # the default since round 6 (Block.default_fp32_mode)
    assert M.set_fp32_mode(enc, "exact") == 3 and all(b.fp32_mode == "exact" for b in enc)
    assert M.set_fp32_mode(model, "3xbf16") == 3 and all(b.fp32_mode == "3xbf16" for b in enc)
    with pytest.raises(M.MetaEncError):
        M.set_fp32_mode(model, "tf32")


def test_tokenizer_parameter_names_match_reference():
    assert list(M.PatchEmbed().state_dict()) == ["proj.weight", "proj.bias"]
    assert M.PatchEmbed().proj.weight.shape == (768, 3, 16, 16)
    assert M.VideoPatchEmbed().proj.weight.shape == (768, 3, 2, 16, 16) and M.VideoPatchEmbed().num_patches == 1568
    assert M.AcousticPatchEmbed.num_tokens(128, 1024) == 1212       # Audio/src/models/ast_models.py:122
    ts = M.DataEmbedding(c_in=7, d_model=64)
    keys = list(ts.state_dict())
    assert "value_embedding.tokenConv.weight" in keys and "position_embedding.pe" in keys
    assert "temporal_embedding.hour_embed.emb.weight" in keys
    assert ts.value_embedding.tokenConv.weight.shape == (64, 7, 3)


def test_flop_model():
    # BASELINE.md section 3
    assert abs(M.encoder_flops_per_sample(197, 768, 12) / 1e9 - 34.895) < 0.01
    assert abs(M.encoder_flops_per_sample(512, 1024, 24) / 1e9 - 335.0) < 0.1


def test_resident_gemm_isa_has_no_inner_loop_spills_and_keeps_its_ticket_register():
    """tools/check_g3r_isa.py on the assembly hipcc emits for gemm3.hip: the hand-counted waits of the resident kernel assume
    that nothing the compiler does not show (a spill, a clobbered ticket register) sits inside its loops."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_g3r_isa", os.path.join(ROOT, "tools", "check_g3r_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        asm = mod.compile_asm(d)
    report, findings = mod.check(asm)
    assert len(report) >= 7 and not findings, findings


def test_attention_backward_isa_keeps_its_ticket_register():
    """The same check on the claimed-item draw of attn_bwd_ring16_kernel (attention.hip): the returning atomic is issued at the head
    of phase A and consumed at its end; nothing may write, spill or copy its result register in between."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_g3r_isa", os.path.join(ROOT, "tools", "check_g3r_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        asm = mod.compile_asm(d, mod.SRC_ATTN)
    report, findings = mod.check(asm, kernel="attn_bwd_ring16_kernel", check_loops=False)
    assert len(report) >= 8 and not findings, findings
    # the 16-wave kernels (ring and streaming forms) are built on four waves per SIMD: <= 128 registers, nothing spilled
    import re
    seen = 0
    for m in re.finditer(r"^(_Z\w*attn_(?:fwd|bwd)\w*(?:ring16|stream16)_kernel\w*):", asm, re.M):
        body = asm[m.start():asm.find(".end_amdhsa_kernel", m.start())]
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        # (the ring backward at head width 64 sits exactly at 128 registers and keeps one 8-byte value in scratch across an item)
        allowed = 4 if "attn_bwd_ring16" in m.group(1) else 0
        assert vgpr <= 128 and body.count("scratch_") <= allowed, (m.group(1), vgpr, body.count("scratch_"))
        seen += 1
    assert seen >= 10, seen      # ring16 forward / backward for every sub-tile count and both head widths, three streaming kernels


def test_fp32_block_that_cannot_run_three_products_says_so_once():
    """fp32_mode = "3xbf16" (default) covers the plain Block; the others run exact fp32 -- with ONE warning per reason, not silently"""
    import warnings
    import torch
    from metatransformer_amd import encoder

    class _B:
        fp32_mode, compute_dtype = "3xbf16", None

    encoder._exact_notes.discard("windowed attention")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        encoder._note_exact_fp32(_B(), torch.float32, torch.float32, "windowed attention")
        encoder._note_exact_fp32(_B(), torch.float32, torch.float32, "windowed attention")        # once
        encoder._note_exact_fp32(_B(), torch.bfloat16, torch.bfloat16, "windowed attention")      # not an fp32 block
        b = _B(); b.fp32_mode = "exact"
        encoder._exact_notes.discard("layer-scale gradient")
        encoder._note_exact_fp32(b, torch.float32, torch.float32, "layer-scale gradient")         # asked for exact: nothing to say
    assert len(w) == 1 and "exact-fp32 kernels" in str(w[0].message) and "windowed attention" in str(w[0].message)
