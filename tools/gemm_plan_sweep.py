"""Host-side sweep of me_gemm descriptors for comparing the GEMM planner of two builds of the library (no GPU needed: the
queries and the planner run on the host, the CU count falls back to 256, and every me_gemm call fails at its launch; `run` hides the GPUs
from its process and refuses to start if one is visible, because the operand addresses it passes are made up).

    python tools/gemm_plan_sweep.py run ROOT OUT      # ROOT: a tree with metatransformer_amd/ and its built libmetaenc.so
    python tools/gemm_plan_sweep.py norm OUT OUT.norm
    python tools/gemm_plan_sweep.py compare A.norm B.norm

`run` writes, per descriptor, a "D" line (the descriptor), a "Q" line (the six public planning queries) and, for me_gemm with and
without a workspace, an "RC" line (return code; the error text of a refusal).  A build made for the comparison additionally prints,
on stderr, one line after planning in gemm_impl and one where the g3 launcher knows its kernel -- they land in OUT between the others:

    PLAN fam=%d bn=%d bm=%d kstep=%d split_k=%d kps=%d ws=%zu tail_rows=%lld tail_split=%d tail_ksteps=%d sk=%d/%d/%d/%d
    FORM kernel=%s epi=%d repi=%d pre=%d G=%d nwg=%d          (kernel: unsupported / resident / one_tile / wrap; with a_wrap_k only
                                                               kernel, epi and nwg)

Those two fprintf lines are a measuring device and are not part of the library.  `norm` writes a refusal for row_stats / row_parts /
ME_GG8 as one line whatever stage made it (me_gemm's argument checks, or a launcher's own late refusal behind its FORM line);
`compare` counts the descriptors whose blocks differ and prints the coverage of the second dump (families, plan branches, forms).
profiles/gemm_plan_equivalence.txt holds the record of the planner refactor made with it."""
import collections, ctypes, itertools, os, re, sys


def run(root, out, limit=None):
    # The operand addresses below are made up: every launch must fail for want of a device.  Hide the GPUs from this process before
    # the HIP runtime is loaded, and refuse to go on if one is visible all the same.
    os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = ""
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    from metatransformer_amd import _capi as C
    assert os.path.dirname(os.path.abspath(C.__file__)).startswith(root), C.__file__
    lib = C.load()
    if lib.me_device_info(0, None, None, None, None, 0) == 0:      # (ME_OK: device 0 exists)
        sys.exit("gemm_plan_sweep: a GPU is visible to this process; the sweep passes made-up addresses to me_gemm and runs without a device only")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)
    def w(s): os.write(2, (s + "\n").encode())
    NT, TN = C.ME_GEMM_NT, C.ME_GEMM_TN
    F32, BF16, F16, X3, X2, GG8 = C.ME_F32, C.ME_BF16, C.ME_F16, C.ME_BF16X3, C.ME_BF16X2, C.ME_GG8
    SAVE, FACTOR = C.ME_GEMM_SAVE_GELU_GRAD, C.ME_GEMM_AUX_IS_FACTOR
    P = lambda i: 0x10000000 * (i + 1)      # fake, 16-byte aligned, distinct operand addresses (never dereferenced on the host)

    def base(op, ab, M, N, K, cdt):
        d = C.GemmDesc()
        d.op, d.ab_dtype, d.M, d.N, d.K = op, ab, M, N, K
        d.A, d.lda = P(0), (K if op == NT else M)
        d.B, d.ldb = P(1), (K if op == NT else N)
        d.C, d.c_dtype, d.alpha = P(2), cdt, 1.0
        d.ldc = N * (3 if cdt == X3 else 2 if cdt == X2 else 1)
        return d
    def bias(d): d.bias = P(3)
    def gelu(d): d.act = C.ME_ACT_GELU
    def preact(dt):
        def f(d): d.preact, d.ldpre, d.preact_dtype = P(4), d.N, dt
        return f
    def aux(dt):
        def f(d): d.aux, d.ldaux, d.aux_dtype = P(5), d.N, dt
        return f
    def res(dt):
        def f(d): d.residual, d.ldres, d.res_dtype = P(6), d.N, dt
        return f
    def flags(v):
        def f(d): d.flags = v
        return f
    def colscale(d): d.colscale = P(7)
    def rowmod(d): d.res_row_mod = 197
    def outgroup(d): d.out_group_rows, d.out_group_stride, d.out_row_offset = 196, 197, 1
    def beta1(d): d.beta = 1.0
    def alpha(d): d.alpha = 0.125
    def affine(d): d.row_affine, d.col_shift = P(8), P(9)
    def parts(d): d.row_parts, d.col_shift, d.row_nparts, d.row_eps = P(8), P(9), max(int(d.K) // 256, 1), 1e-6
    def stats(d): d.row_stats = P(10)
    def wrap(d):      # K = 3 Kc: A = [hi | lo] planes of Kc columns each
        kc = int(d.K) // 3
        d.a_wrap_k, d.lda = 2 * kc, 2 * kc
    def colsum(d): d.colsum_a = P(11)
    def wide_ld(d): d.ldc = (1 << 22) + 8      # 256 * ldc * 2 >= 2^31: past the resident kernel's 32-bit tile offsets
    EPI_NT = {
        "plain": [], "bias": [bias], "bias_gelu": [bias, gelu], "bias_gelu_preact_bf16": [bias, gelu, preact(BF16)], "bias_gelu_preact_f32": [bias, gelu, preact(F32)],
        "save_gg_bf16": [bias, gelu, preact(BF16), flags(SAVE)], "save_gg_f32": [bias, gelu, preact(F32), flags(SAVE)], "save_gg_gg8": [bias, gelu, preact(GG8), flags(SAVE)],
        "aux_bf16": [aux(BF16)], "aux_f32": [aux(F32)], "factor_bf16": [aux(BF16), flags(FACTOR)], "factor_f32": [aux(F32), flags(FACTOR)], "factor_gg8": [aux(GG8), flags(FACTOR)],
        "res_bf16": [bias, res(BF16)], "res_f32": [bias, res(F32)], "res_bf16_colscale": [bias, res(BF16), colscale], "res_f32_colscale": [bias, res(F32), colscale],
        "colscale": [bias, colscale], "gelu_colscale": [bias, gelu, colscale], "res_rowmod": [res(BF16), rowmod], "outgroup": [bias, outgroup], "beta1": [beta1], "alpha": [alpha],
        "alpha_res": [alpha, res(BF16)], "affine": [bias, affine], "affine_gelu": [bias, gelu, affine], "affine_res": [bias, affine, res(BF16)],
        "parts": [bias, parts], "parts_gelu": [bias, gelu, parts], "parts_res": [bias, parts, res(BF16)],
        "stats": [bias, res(BF16), stats], "stats_colscale": [bias, res(BF16), colscale, stats], "stats_f32res": [bias, res(F32), stats], "stats_gelu": [bias, gelu, res(BF16), stats],
        "wrap": [bias, wrap], "wrap_res_f32": [bias, res(F32), wrap], "wrap_gelu": [bias, gelu, wrap], "wrap_gelu_colscale": [bias, gelu, colscale, wrap], "wrap_res_bf16": [bias, res(BF16), wrap],
        "wrap_parts": [bias, parts, wrap], "wrap_stats": [bias, res(BF16), stats, wrap], "wrap_gg8": [bias, gelu, preact(GG8), flags(SAVE), wrap],
        "save_gg8_res": [bias, gelu, preact(GG8), flags(SAVE), res(BF16)], "gg8_alpha": [aux(GG8), flags(FACTOR), alpha],
        "wide_ldc": [bias, wide_ld], "wide_ldc_parts": [bias, parts, wide_ld],
    }
    EPI_TN = {"plain": [], "beta1": [beta1], "colsum": [colsum], "colsum_beta1": [colsum, beta1], "alpha": [alpha], "bias": [bias]}
    Ms = [128, 197, 256, 512, 3072, 4096, 6304, 8192, 8224, 50176 + 7, 50432, 65536]
    Ns = [64, 128, 384, 768, 1024, 2304, 3072, 4096, 772, 776]      # (776: a multiple of 8, not of 128 -- the g2w family)
    Ks = [64, 200, 384, 768, 1024, 1280, 2304, 3072, 4096, 9216]
    WO = [64, 128, 384, 768, 1024, 2304, 3072, 4096, 776]       # TN: output features on both sides
    TOK = [197, 200, 3072, 4096, 6304, 8224, 50176 + 8, 50432, 65536]
    def cases():
        for M, N, K in itertools.product(Ms, Ns, Ks):
            for cdt in (BF16, F32, X2, X3, F16):
                for name, mods in EPI_NT.items():
                    yield NT, BF16, M, N, K, cdt, name, mods
            for cdt in (BF16, F32):
                for name in ("plain", "bias_gelu", "res_f32", "res_bf16", "parts", "stats"):
                    yield NT, F32, M, N, K, cdt, name, EPI_NT[name]
        for M, N, K in itertools.product(WO, WO, TOK):
            for ab in (BF16, F32):
                for cdt in (F32, BF16):
                    for name, mods in EPI_TN.items():
                        yield TN, ab, M, N, K, cdt, name, mods
    WS = 1 << 42
    n = 0
    for reserve in (0, 16):
        prev = lib.me_gemm_reserve_cus(reserve)
        for op, ab, M, N, K, cdt, name, mods in cases():
            if reserve and op == NT and not (name in ("plain", "res_bf16", "parts", "stats", "save_gg_gg8", "wrap") and cdt in (BF16, F32)): continue      # (the reservation only enters the wgrad plan)
            d = base(op, ab, M, N, K, cdt)
            for f in mods: f(d)
            r = ctypes.byref(d)
            w(f"D r={reserve} op={op} ab={ab} M={M} N={N} K={K} cdt={cdt} epi={name}")
            w(f"Q ws={lib.me_gemm_workspace_bytes(r)} colsum={lib.me_gemm_fuses_colsum(r)} stats={lib.me_gemm_emits_row_stats(r)} parts={lib.me_gemm_takes_row_parts(r)} "
              f"wrap={lib.me_gemm_takes_a_wrap(r)} gg8={lib.me_gemm_takes_gg8(r)}")
            for ws in (WS, 0):
                d.workspace, d.workspace_bytes = (P(12), ws) if ws else (None, 0)
                rc = lib.me_gemm(r, None)
                w(f"RC ws={int(bool(ws))} rc={rc}" + (f" err={lib.me_last_error().decode()}" if rc in (-1, -2) else ""))
            n += 1
            if limit and n >= limit: break
        lib.me_gemm_reserve_cus(prev)
        if limit and n >= limit: break
    w(f"END {n} descriptors")


FEATURES = [("row_stats", "row_stats"), ("row_parts", "row_parts"), ("ME_GG8", "gg8")]


def norm(src, dst):
    out = []
    for line in open(src):
        line = line.rstrip("\n")
        if line.startswith("RC ") and (" rc=-1 " in line or " rc=-2 " in line):
            err = line.split("err=", 1)[1]
            for key, name in FEATURES:
                if err.startswith("me_gemm: " + key + " ") and ("is not available" in err or "needs the resident" in err):
                    if out and out[-1].startswith("FORM kernel=unsupported"):
                        out.pop()
                    line = line.split(" rc=")[0] + " REFUSED " + name
                    break
        out.append(line)
    open(dst, "w").write("\n".join(out) + "\n")


def blocks(path):
    cur = None
    for line in open(path):
        if line.startswith("D "):
            if cur:
                yield cur
            cur = [line.rstrip()]
        elif cur is not None:
            cur.append(line.rstrip())
    if cur:
        yield cur


def compare(a_path, b_path):
    n = differ = 0
    fam, plan, form, refused, yes = (collections.Counter() for _ in range(5))
    for a, b in zip(blocks(a_path), blocks(b_path)):
        n += 1
        assert a[0] == b[0], (a[0], b[0])
        if a != b:
            differ += 1
            if differ <= 10:
                print("DIFFERS", a[0], "\n   ", [x for x in a[1:] if x not in b], "\n   ", [x for x in b[1:] if x not in a])
        first = True
        for line in b[1:]:
            if line.startswith("PLAN") and first:
                first = False
                m = dict(kv.split("=") for kv in line.split()[1:])
                fam[m["fam"]] += 1
                plan["fam" + m["fam"] + ("/bm%s_bn%s" % (m["bm"], m["bn"]) if m["fam"] == "2" else "") + ("/splitk" if int(m["split_k"]) > 1 else "")
                     + ("/tail" if int(m["tail_rows"]) > 0 else "") + ("/balanced" if not m["sk"].startswith("0/") else "")] += 1
            elif line.startswith("FORM"):
                m = dict(kv.split("=") for kv in line.split()[1:])
                form[(m["kernel"], "epi=" + m["epi"]) if m["kernel"] != "resident" else ("resident", "repi=" + m["repi"], "pre=" + m["pre"])] += 1
            elif "REFUSED" in line:
                refused[line.split("REFUSED ")[1].strip()] += 1
            elif line.startswith("Q "):
                for kv in line.split()[1:]:
                    k, v = kv.split("=")
                    if v != "0":
                        yes[k] += 1
    print(n, "descriptors;", differ, "differ")
    print("family of the plan (valid descriptors):", dict(sorted(fam.items())))
    print("plan branches:", dict(sorted(plan.items())))
    print("g3 forms per launch:")
    for k, v in sorted(form.items()):
        print("   ", k, v)
    print("refused at the capability checks (per call):", dict(refused))
    print("queries answering yes:", dict(yes))
    return differ


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else None)
    elif cmd == "norm":
        norm(sys.argv[2], sys.argv[3])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
