"""CPU: the C-ABI library loads, exports every symbol include/deseq2_mi355x.h declares, and
fails loudly (no CPU fallback) when no GPU is present; the ctypes binding (deseq2_amd/_lib.py) is held whole to the header:
every struct layout, every signature, every constant.  No compute calls here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/deseq2_mi355x.h without its comments"""
    h = open(os.path.join(ROOT, "include", "deseq2_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", h, flags=re.S)


def _header_symbols():
    return sorted(set(re.findall(r"\b(dsq_[a-z0-9_]+)\s*\(", _header())))


def test_library_exports_every_declared_symbol():
    from deseq2_amd import _lib
    L = _lib.lib()
    syms = _header_symbols()
    assert len(syms) >= 16
    assert sorted(_lib.EXPORTED_SYMBOLS) == syms
    for s in syms:
        assert hasattr(L, s), "missing export " + s
    assert L.dsq_version() == 100


# ---- deseq2_amd/_lib.py against the header: layouts, signatures, constants.  gcc and the header only, no built library ----
def _compiled(statements):
    """the lines a C program of these statements prints, compiled against the header"""
    import subprocess
    import tempfile
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "deseq2_mi355x.h"\n#define SZ(T, f) sizeof(((T *)0)->f)\n'
           'int main(void){\n%s\nreturn 0; }\n' % "\n".join(statements))
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        return subprocess.check_output([exe]).decode().strip().splitlines()


def test_struct_layout_matches_header():
    """every block the header defines has its ctypes mirror and no other exists: size, and the offset and size of every
    field, as the C compiler lays them out; the last field mirrored ends where the block ends, so that a field missing at
    the tail fails even where padding would hide it"""
    from deseq2_amd import _lib
    names = re.findall(r"\}\s*(Dsq\w+)\s*;", _header())
    assert len(names) >= 46 and len(set(names)) == len(names)
    mirrors = {v.__name__ for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)
               and v.__name__.startswith("Dsq")}
    assert mirrors == set(names), sorted(mirrors ^ set(names))
    lines = []
    for nm in names:
        t = getattr(_lib, nm)
        assert t.__name__ == nm
        lines.append('printf("%%zu %%zu", sizeof(%s), _Alignof(%s));' % (nm, nm))
        for f, _ in t._fields_:
            c = "lambda" if f == "lambda_" else f
            lines.append('printf(" %%zu %%zu", offsetof(%s, %s), SZ(%s, %s));' % (nm, c, nm, c))
        lines.append('printf("\\n");')
    out = _compiled(lines)
    assert len(out) == len(names)
    for nm, line in zip(names, out):
        t = getattr(_lib, nm)
        size, align, *fields = map(int, line.split())
        want = [ctypes.sizeof(t), ctypes.alignment(t)] + [v for f, _ in t._fields_ for v in (getattr(t, f).offset, getattr(t, f).size)]
        assert [size, align] + fields == want, nm
        end = fields[-2] + fields[-1]
        assert -(-end // align) * align == size, "%s: fields are missing behind %s" % (nm, t._fields_[-1][0])


def _prototypes():
    """{name: (return type, [parameter types])} of every function the header declares, as C spells them"""
    protos = {}
    for ret, name, params in re.findall(r"^[ \t]*((?:const\s+)?\w+(?:\s*\*)?)\s*\b(dsq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M):
        assert name not in protos, name
        params = [" ".join(q.split()) for q in params.split(",")]
        protos[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return protos


def _ctype_of(c_type, _lib, is_return=False):
    """the ctypes type(s) that may stand for a C parameter (its name still attached) or return type"""
    scalars = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    if "*" in c_type:
        base = c_type[:c_type.index("*")].replace("const", "").strip()
        if base.startswith("Dsq"):
            return (ctypes.POINTER(getattr(_lib, base)),)
        if is_return:
            assert base == "char", c_type
            return (ctypes.c_char_p,)
        return (ctypes.c_void_p, ctypes.c_char_p)
    base = c_type if is_return else c_type.rsplit(" ", 1)[0]          # `int32_t n` -> int32_t
    return (scalars[base],)


def test_signatures_match_header():
    """the signature table names the functions the header declares, each with the prototype's parameter count, scalar widths,
    argument blocks and return type"""
    from deseq2_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == _header_symbols() and len(protos) >= 83           # no prototype escaped the strict pattern
    assert sorted(_lib.SIGNATURES) == sorted(protos)
    assert _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES)
    assert {"dsq_pt_dev", "dsq_weights_prep_dev", "dsq_beta_prior_var_dev"} <= set(protos)      # the multi-line ones
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert argtypes is not None and len(argtypes) == len(params), name
        assert restype in _ctype_of(ret, _lib, is_return=True), (name, ret, restype)
        for i, (c_type, t) in enumerate(zip(params, argtypes)):
            assert t in _ctype_of(c_type, _lib), (name, i, c_type, t)


def _c_spelling(key):
    """the header's spelling of a key of the Python-side families: upper case, camel humps split"""
    s = re.sub(r"([A-Z][a-z]+)(?=\d)", r"\1_", key)       # a number behind a hump is one of its own: Abs2014 -> Abs_2014
    return re.sub(r"(?<=[a-z])(?=[A-Z])", "_", s).upper()


# header constants that Python deliberately does not mirror
_NOT_MIRRORED = {"DSQ_VERSION": "the library reports it: dsq_version() is held to 100 in test_library_exports_every_declared_symbol"}


def test_constants_match_header():
    """from the header to Python: every DSQ_* macro and enumerator, with the value the C compiler gives it, is mirrored by
    exactly one rule -- a module attribute of its name or a key of its family's dict -- or is exempted by name"""
    from deseq2_amd import _lib
    assert [_c_spelling(k) for k in ("greaterAbs2014", "two_sided", "Wald", "LRT", "dist2", "parametric_or_mean")] == [
        "GREATER_ABS_2014", "TWO_SIDED", "WALD", "LRT", "DIST2", "PARAMETRIC_OR_MEAN"]
    h = _header()
    names = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DSQ_\w+)[ \t]+\S", h, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", h):
        names += re.findall(r"\b(DSQ_\w+)\b", body)
    assert len(names) >= 70 and len(set(names)) == len(names)
    out = _compiled(['printf("%%lld\\n", (long long)(%s));' % nm for nm in names])
    header = dict(zip(names, map(int, out)))
    assert len(out) == len(names)
    # (prefix, dict): key k mirrors <prefix>_<_c_spelling(k)>; DSQ_FPM is the irregular family: DSQ_FPM, DSQ_FPKM_*
    families = [("DSQ_" + f, getattr(_lib, "DSQ_" + f)) for f in ("TEST", "ALT", "PT", "VST", "SF", "PAIRS", "FIT", "ST")]
    families.append(("DSQ", _lib.DSQ_FPM))
    mirror = {}
    for prefix, d in families:
        for k, v in d.items():
            mirror.setdefault(prefix + "_" + _c_spelling(k), []).append(v)
    assert set(mirror) <= set(header), sorted(set(mirror) - set(header))         # no key without its constant
    for nm in header:
        claims = list(mirror.get(nm, []))
        if isinstance(getattr(_lib, nm, None), int):
            claims.append(getattr(_lib, nm))
        if nm in _NOT_MIRRORED:
            assert not claims, nm
            continue
        assert len(claims) == 1, "%s is mirrored %d times" % (nm, len(claims))
        assert claims[0] == header[nm], (nm, claims[0], header[nm])
    assert set(_NOT_MIRRORED) <= set(header)
    assert header["DSQ_VERSION"] == 100
    assert _lib.ERR_NAMES == {v: nm for nm, v in header.items() if nm.startswith("DSQ_ERR_")}
    # every module-level DSQ_* integer is one of the header's, too
    assert {k for k, v in vars(_lib).items() if k.startswith("DSQ_") and isinstance(v, int)} <= set(header)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from deseq2_amd import _lib, native
    y = np.ones((4, 6), dtype=np.int32)
    x = np.column_stack([np.ones(6), np.repeat([0, 1], 3)]).astype(float)
    with pytest.raises(_lib.DsqError) as ei:
        native.fitBeta(y, x, np.ones((4, 6)), np.full(4, 0.1), [1, 0], np.zeros((4, 2)), [1e-6, 1e-6],
                       np.ones((4, 6)), False, 1e-8, 100, True, 0.5)
    assert ei.value.code == 3            # DSQ_ERR_DEVICE
    with pytest.raises(_lib.DsqError):
        native.fitDisp(y, x, np.ones((4, 6)), np.zeros(4), np.zeros(4), 1.0, -20.0, 1.0, 1e-6, 100, False,
                       np.ones((4, 6)), False, 1e-2, True)


def test_argument_validation():
    from deseq2_amd import native
    y = np.ones((4, 6), dtype=np.int32)
    x = np.ones((5, 2))
    with pytest.raises(ValueError):
        native.fitBeta(y, x, np.ones((4, 6)), np.full(4, 0.1), [1, 0], np.zeros((4, 2)), [1e-6, 1e-6],
                       np.ones((4, 6)), False, 1e-8, 100, True, 0.5)


# dsq_deseq_workspace_bytes(n, 12, p, n_trend) as the library of commit b05cb59 (the one before the workspace layout became
# one table in pipeline.hip) returns it: per p, the pairs (n_trend = n // 2, n_trend = 2 n + 3) for n = 1, 7, 6 250, 50 000
_WORKSPACE_BYTES = {
    1: (3008, 3008, 3008, 3392, 1802432, 1952384, 14400704, 15600896),
    4: (3072, 3072, 4800, 5184, 3152064, 3302016, 25200768, 26400960),
    10: (3776, 3776, 7808, 8192, 5852480, 6002432, 46800896, 48001088),
    11: (3904, 3904, 10816, 11200, 8552320, 8702272, 68401024, 69601216),
    31: (5440, 5440, 19264, 19648, 15752704, 15902656, 126001408, 127201600),
    48: (6976, 6976, 27712, 28096, 22953088, 23103040, 183601792, 184801984),
    64: (8512, 8512, 36160, 36544, 30153472, 30303424, 241202176, 242402368),
}


@pytest.mark.parametrize("p", sorted(_WORKSPACE_BYTES))
def test_deseq_workspace_bytes_is_pinned(p):
    """the caller-owned workspace of dsq_deseq_dev persists between the phases of an analysis: its size is ABI (pure host
    code -- the library loads without a device)"""
    from deseq2_amd import _lib
    L = _lib.lib()
    got = tuple(int(L.dsq_deseq_workspace_bytes(n, 12, p, nt)) for n in (1, 7, 6250, 50000) for nt in (n // 2, 2 * n + 3))
    assert got == _WORKSPACE_BYTES[p]
    assert L.dsq_deseq_workspace_bytes(0, 12, p, 0) == 0 and L.dsq_deseq_workspace_bytes(7, 12, 0, 0) == 0


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: nothing under deseq2_amd/ may reference it"""
    for dp, _, files in os.walk(os.path.join(ROOT, "deseq2_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".c", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "import oracle" not in txt and "from oracle" not in txt and "orc_" not in txt, f


def test_r_shim_compiles_warning_free_against_the_mock_r_headers():
    """R is not installed here: the .Call shim is compiled (gcc -Wall -Wextra -Werror, no link) against the mock R API of
    tests/r_mock/ -- tests/test_r_shim.py then EXECUTES it on that mock runtime"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-cast-function-type", "-Werror", "-DDSQ_HAVE_R",
                        "-I", os.path.join(root, "tests", "r_mock"),
                        "-I", os.path.join(root, "include"), os.path.join(root, "deseq2_amd", "csrc", "r_shim.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("case", ["standard_two_group", "standard_two_factors", "expanded_three_levels", "expanded_two_factors",
                                  "ties_and_zero_rows"])
def test_beta_prior_var_equals_the_host_mirror(case):
    """dsq_beta_prior_var (csrc/beta_prior.hip: estimateBetaPriorVar of R/core.R:1601-1689 inside the library, pure host
    code -- runs without a GPU) against core.estimateBetaPriorVar, the line-cited mirror: same stable order, same
    sequential sums, so the same bits."""
    from deseq2_amd import core, native
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, case))))
    n = 3000
    if case in ("standard_two_group",):
        factors = {"condition": np.repeat([0, 1], 4)}
    elif case in ("expanded_three_levels", "ties_and_zero_rows"):
        factors = {"condition": np.repeat([0, 1, 2], 3)}
    else:
        factors = {"batch": np.tile([0, 1, 2], 4), "condition": np.repeat([0, 1, 2, 3], 3)}
    x, names = core.standard_model_matrix(factors)
    p = x.shape[1]
    mle = rng.normal(0, 1.5, (n, p)) * rng.choice([1.0, 1.0, 1.0, 8.0], (n, 1))       # some |beta| >= 10
    mle[:, 0] = rng.normal(5, 2, n)
    bm = np.exp(rng.normal(3, 2, n))
    dfit = 0.05 + 3.0 / bm
    az = np.zeros(n, bool)
    if case == "ties_and_zero_rows":
        mle[::7, 1] = 0.25                                     # exact ties of |beta| ...
        mle[1::7, 1] = -0.25                                   # ... across signs
        mle[::11, 2] = np.nan                                  # rows without a coefficient
        az[::13] = True
    expanded = case.startswith("expanded") or case == "ties_and_zero_rows"
    mmt = "expanded" if expanded else "standard"
    view = type("V", (), {"mcols": {"baseMean": bm[~az], "dispFit": dfit[~az]}})()
    ref, _ = core.estimateBetaPriorVar(view, mle[~az], names, modelMatrixType=mmt, factors=factors)
    got = native.estimateBetaPriorVarHost(
        mle, bm, dfit, az, native.coef_factor_codes(factors),
        prior_coef_factor=native.coef_factor_codes(factors, expanded=True) if expanded else None)
    assert got.shape == np.asarray(ref).shape
    assert (got == np.asarray(ref)).all(), (got, ref)
    assert got[0] == 1e6 and (got > 0).all()


def test_beta_prior_var_of_a_one_gene_object():
    """nrow(betaMatrix) == 1 (R/core.R:1647,1662): the prior variances are the squared coefficients themselves (the
    intercept still 1e6, :1669-1671) -- library and mirror alike"""
    from deseq2_amd import core, native
    factors = {"condition": np.repeat([0, 1], 4)}
    x, names = core.standard_model_matrix(factors)
    mle = np.array([[5.0, -1.75], [np.nan, np.nan]])
    bm, dfit, az = np.array([30.0, 0.0]), np.array([0.2, 0.2]), np.array([False, True])       # the second row is all zero
    view = type("V", (), {"mcols": {"baseMean": bm[~az], "dispFit": dfit[~az]}})()
    ref, _ = core.estimateBetaPriorVar(view, mle[~az], names, modelMatrixType="standard", factors=factors)
    got = native.estimateBetaPriorVarHost(mle, bm, dfit, az, native.coef_factor_codes(factors))
    assert list(ref) == [1e6, 1.75 ** 2] and list(got) == [1e6, 1.75 ** 2]


def test_shipped_library_passes_the_exec_lint():
    """profiles/r04_exec_remat.md: the toolchain can re-materialise a constant above the exec restore of a join block (it
    did, in two kernels of round 4: sqrt() returned its argument).  tools/exec_lint.py looks for that pattern in the
    disassembly of every gfx950 code object of the library that ships."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lint = os.path.join(root, "tools", "exec_lint.py")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    from deseq2_amd import _lib
    r = subprocess.run([sys.executable, lint, _lib.SO_PATH], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "0 suspicious" in r.stdout


def test_exec_lint_flags_the_round_4_pattern_and_not_a_masked_body():
    """the lint on three synthetic disassemblies: (a) round 4's defect -- constants of the next statement written at the
    fall-through of a lane-dependent loop latch, above the exec restore; (b) a constant at the target of a forward
    s_cbranch_execz, above the restore; (c) the body of a masked region entered through a forward s_cbranch_execnz (the
    weighted fit_disp<4>'s `pivot = 1.0` of a dropped column): legitimate, not reported."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("exec_lint", os.path.join(root, "tools", "exec_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)

    def dis(rows, base=0x1000):
        out = ["%016x <k>:" % base]
        for i, r in enumerate(rows):
            out.append("\t%-60s// %012X: 00000000%s" % (r[0], base + 4 * i, "" if len(r) < 2 else " <k+0x%x>" % (4 * r[1])))
        return "\n".join(out)

    a = dis([("v_add_f64 v[0:1], v[0:1], v[2:3]",), ("s_andn2_b64 exec, exec, s[2:3]",), ("s_cbranch_execnz 65533", 0),
             ("s_mov_b32 s80, 0",), ("v_mov_b32_e32 v116, 0x260",), ("s_or_b64 exec, exec, s[0:1]",), ("s_endpgm",)])
    b = dis([("s_and_saveexec_b64 s[8:9], vcc",), ("s_cbranch_execz 2", 3), ("v_add_f64 v[0:1], v[0:1], v[2:3]",),
             ("v_mov_b64_e32 v[4:5], 1.0",), ("s_or_b64 exec, exec, s[8:9]",), ("s_endpgm",)])
    c = dis([("s_and_saveexec_b64 s[8:9], s[0:1]",), ("s_cbranch_execnz 1", 3), ("s_branch 1", 4),
             ("v_mov_b64_e32 v[60:61], 1.0",), ("s_or_b64 exec, exec, s[8:9]",), ("s_endpgm",)])
    hits = [[t for _, _, t in lint.scan(lint.blocks_of_disassembly(x, "t"))] for x in (a, b, c)]
    assert hits[0] == ["v_mov_b32_e32 v116, 0x260"], hits
    assert hits[1] == ["v_mov_b64_e32 v[4:5], 1.0"], hits
    assert hits[2] == [], hits


# ---- status codes of the argument checks ---------------------------------------------------------------------------------
def _tiny_blocks():
    """valid argument blocks of every block-taking entry at n = 4, m = 6, p = 2 (tests/capi_blocks.py)"""
    from tests import capi_blocks
    from tests.helpers import make_case
    d = make_case(40, 6, "two_group", seed=5)
    d = {k: (v[:4] if isinstance(v, np.ndarray) and v.shape[:1] == d["counts"].shape[:1] else v) for k, v in d.items()}
    B = capi_blocks.blocks(d)
    for k in ("fit_beta", "fit_disp", "fit_disp_grid", "prefit_moments", "nbinom_loglike", "intercept_fit", "optim_rows"):
        B[k].inputs["weights"] = np.ones((4, 6))           # given but unused: `useWeights without weights` NULLs it
    return B


def _argument_cases():
    """(case id, thunk returning the status code): from each valid block, one thing broken at a time"""
    import ctypes as C
    from deseq2_amd import _lib
    from tests import capi_blocks as cb
    L = _lib.lib()
    cases = []
    B = _tiny_blocks()
    for key, b in B.items():
        entries = [(b.name, "host")] + ([(b.name + "_rows", "rows")] if key.startswith("fit_") else [])
        if key == "vst":
            entries += [("dsq_vst_dev", "dev"), ("dsq_vst_rowstats_dev", "dev")]
        elif b.dev:
            entries.append((b.dev, "dev"))
        for ename, how in entries:
            def run(blk, null_args=False, null_out=False, ename=ename, how=how):
                keep = {k: (None if v is None else cb.fcol(v)) for k, v in blk.inputs.items()}
                outs = {k: np.zeros(shape, dtype=dt, order="F") for k, (shape, dt) in blk.outputs.items()}
                a = blk.args({k: cb.ptr(v) for k, v in keep.items()})
                tail = {"host": (), "rows": (0, 4), "dev": (None,)}[how]
                fn = getattr(L, ename)
                pa = None if null_args else C.byref(a)
                optr = {k: cb.ptr(v) for k, v in outs.items()}
                if blk.style == "mu":
                    return fn(pa, 0.5, None if null_out else optr["mu"], *tail)
                if blk.style == "vec":
                    return fn(pa, None if null_out else optr["loglike"], *tail)
                o = blk.O(**optr, **blk.out_scalars)
                return fn(pa, None if null_out else C.byref(o), *tail)

            def add(what, blk, run=run, ename=ename, **kw):
                cases.append(("%s: %s" % (ename, what), lambda blk=blk, kw=kw, run=run: run(blk, **kw)))
            add("NULL args", b, null_args=True)
            add("NULL out", b, null_out=True)
            for f in b.inputs:
                if b.inputs[f] is not None:
                    add("args.%s NULL" % f.rstrip("_"), b.but(**{f: None}))
            if b.style == "ao":
                for f in b.outputs:
                    add("out.%s NULL" % f, b.but(drop_out=[f]))
            add("n = -1", b.but(n=-1))
            add("m = 0", b.but(m=0))
            if "p" in b.scalars:
                add("p = 0", b.but(p=0))
                add("p = 65", b.but(p=65))
            if "useWeights" in b.scalars and "weights" in b.inputs and key != "linear_mu":
                add("useWeights without weights", b.but(useWeights=1, weights=None))
            if "maxit" in b.scalars:
                add("maxit = -1", b.but(maxit=-1))
            if "ngrid" in b.scalars:
                add("ngrid = 1", b.but(ngrid=1))
            if "trim" in b.scalars:
                add("trim = 0.5", b.but(trim=0.5))
            add("y_type = 7", b.but(y_type=7))
            if "type" in b.scalars:
                add("type = 9", b.but(type=9))
            if "kind" in b.scalars:
                add("kind = 9", b.but(kind=9))
            if key == "prefit_moments":
                add("m <= p", b.but(p=6))
            if key == "cooks_distance":
                add("ncell = 0", b.but(ncell=0))
            if how == "dev":
                add("gene-major, ld < m", b.but(layout=1, ld=5))
                add("layout = 7", b.but(layout=7, ld=8))
            else:
                add("layout = GENE_MAJOR", b.but(layout=1, ld=8))
            if how == "rows":
                cases.append(("%s: row range past n" % ename, lambda b=b, ename=ename: cb._invoke(
                    b, getattr(L, ename), b.args({k: cb.ptr(None if v is None else cb.fcol(v)) for k, v in b.inputs.items()}),
                    {k: None for k in b.outputs}, (2, 3))))
    # the entries that take plain arguments
    v = np.ones(8)
    i4 = np.ones(8, np.int32)
    P = cb.ptr
    plain = {
        "dsq_parametric_dispersion_fit": lambda **k: L.dsq_parametric_dispersion_fit(
            k.get("means", P(v)), P(v), k.get("n", 8), k.get("coefs", P(v)), P(i4)),
        "dsq_parametric_dispersion_fit_dev": lambda **k: L.dsq_parametric_dispersion_fit_dev(
            k.get("means", P(v)), P(v), k.get("n", 8), k.get("coefs", P(v)), P(i4), None),
        "dsq_test_math": lambda **k: L.dsq_test_math(k.get("op", 0), k.get("means", P(v)), k.get("b"), None, k.get("coefs", P(v)),
                                                     k.get("n", 8)),
    }
    for ename, f in plain.items():
        cases.append((ename + ": first input NULL", lambda f=f: f(means=None)))
        cases.append((ename + ": output NULL", lambda f=f: f(coefs=None)))
        cases.append((ename + ": n = -1", lambda f=f: f(n=-1)))
    cases.append(("dsq_parametric_dispersion_fit: n = 0", lambda: plain["dsq_parametric_dispersion_fit"](n=0)))
    cases.append(("dsq_parametric_dispersion_fit_dev: n = 0", lambda: plain["dsq_parametric_dispersion_fit_dev"](n=0)))
    cases.append(("dsq_test_math: op 7 without b", lambda: plain["dsq_test_math"](op=7)))
    for op in (8, 10, 11, 15, 17, 22):
        cases.append(("dsq_test_math: op %d without b" % op, lambda op=op: plain["dsq_test_math"](op=op)))
    for op in (8, 22):
        cases.append(("dsq_test_math: op %d with b, without c" % op, lambda op=op: plain["dsq_test_math"](op=op, b=P(v))))
    return cases


# the status code of each case as the library of commit e1d44e3 (the parent of the change that states every call's checks
# once, check_<call> of csrc/capi.hip) returns it.  Only the cases that library decides BEFORE it looks for a device are
# listed (1 = DSQ_ERR_ARG, 2 = DSQ_ERR_UNSUPPORTED), so the table holds with and without a GPU.
_ARGUMENT_CODES = {
    'dsq_fit_beta: NULL args': 1,
    'dsq_fit_beta: NULL out': 1,
    'dsq_fit_beta: args.y NULL': 1,
    'dsq_fit_beta: args.x NULL': 1,
    'dsq_fit_beta: args.nf NULL': 1,
    'dsq_fit_beta: args.alpha_hat NULL': 1,
    'dsq_fit_beta: args.contrast NULL': 1,
    'dsq_fit_beta: args.beta_mat NULL': 1,
    'dsq_fit_beta: args.lambda NULL': 1,
    'dsq_fit_beta: out.beta_mat NULL': 1,
    'dsq_fit_beta: out.beta_var_mat NULL': 1,
    'dsq_fit_beta: out.iter NULL': 1,
    'dsq_fit_beta: out.contrast_num NULL': 1,
    'dsq_fit_beta: out.contrast_denom NULL': 1,
    'dsq_fit_beta: out.deviance NULL': 1,
    'dsq_fit_beta: n = -1': 1,
    'dsq_fit_beta: m = 0': 1,
    'dsq_fit_beta: p = 0': 1,
    'dsq_fit_beta: useWeights without weights': 1,
    'dsq_fit_beta: layout = GENE_MAJOR': 1,
    'dsq_fit_beta_rows: NULL args': 1,
    'dsq_fit_beta_rows: NULL out': 1,
    'dsq_fit_beta_rows: args.y NULL': 1,
    'dsq_fit_beta_rows: args.x NULL': 1,
    'dsq_fit_beta_rows: args.nf NULL': 1,
    'dsq_fit_beta_rows: args.alpha_hat NULL': 1,
    'dsq_fit_beta_rows: args.contrast NULL': 1,
    'dsq_fit_beta_rows: args.beta_mat NULL': 1,
    'dsq_fit_beta_rows: args.lambda NULL': 1,
    'dsq_fit_beta_rows: out.beta_mat NULL': 1,
    'dsq_fit_beta_rows: out.beta_var_mat NULL': 1,
    'dsq_fit_beta_rows: out.iter NULL': 1,
    'dsq_fit_beta_rows: out.contrast_num NULL': 1,
    'dsq_fit_beta_rows: out.contrast_denom NULL': 1,
    'dsq_fit_beta_rows: out.deviance NULL': 1,
    'dsq_fit_beta_rows: n = -1': 1,
    'dsq_fit_beta_rows: m = 0': 1,
    'dsq_fit_beta_rows: p = 0': 1,
    'dsq_fit_beta_rows: useWeights without weights': 1,
    'dsq_fit_beta_rows: layout = GENE_MAJOR': 1,
    'dsq_fit_beta_rows: row range past n': 1,
    'dsq_fit_beta_dev: NULL args': 1,
    'dsq_fit_beta_dev: NULL out': 1,
    'dsq_fit_beta_dev: args.y NULL': 1,
    'dsq_fit_beta_dev: args.x NULL': 1,
    'dsq_fit_beta_dev: args.nf NULL': 1,
    'dsq_fit_beta_dev: args.alpha_hat NULL': 1,
    'dsq_fit_beta_dev: args.contrast NULL': 1,
    'dsq_fit_beta_dev: args.beta_mat NULL': 1,
    'dsq_fit_beta_dev: args.lambda NULL': 1,
    'dsq_fit_beta_dev: out.beta_mat NULL': 1,
    'dsq_fit_beta_dev: out.beta_var_mat NULL': 1,
    'dsq_fit_beta_dev: out.iter NULL': 1,
    'dsq_fit_beta_dev: out.contrast_num NULL': 1,
    'dsq_fit_beta_dev: out.contrast_denom NULL': 1,
    'dsq_fit_beta_dev: out.deviance NULL': 1,
    'dsq_fit_beta_dev: n = -1': 1,
    'dsq_fit_beta_dev: m = 0': 1,
    'dsq_fit_beta_dev: p = 0': 1,
    'dsq_fit_beta_dev: p = 65': 2,
    'dsq_fit_beta_dev: useWeights without weights': 1,
    'dsq_fit_beta_dev: maxit = -1': 1,
    'dsq_fit_beta_dev: gene-major, ld < m': 1,
    'dsq_fit_beta_dev: layout = 7': 1,
    'dsq_fit_disp: NULL args': 1,
    'dsq_fit_disp: NULL out': 1,
    'dsq_fit_disp: args.y NULL': 1,
    'dsq_fit_disp: args.x NULL': 1,
    'dsq_fit_disp: args.mu_hat NULL': 1,
    'dsq_fit_disp: args.log_alpha NULL': 1,
    'dsq_fit_disp: args.log_alpha_prior_mean NULL': 1,
    'dsq_fit_disp: out.log_alpha NULL': 1,
    'dsq_fit_disp: out.last_change NULL': 1,
    'dsq_fit_disp: out.initial_lp NULL': 1,
    'dsq_fit_disp: out.initial_dlp NULL': 1,
    'dsq_fit_disp: out.last_lp NULL': 1,
    'dsq_fit_disp: out.last_dlp NULL': 1,
    'dsq_fit_disp: out.last_d2lp NULL': 1,
    'dsq_fit_disp: out.iter NULL': 1,
    'dsq_fit_disp: out.iter_accept NULL': 1,
    'dsq_fit_disp: n = -1': 1,
    'dsq_fit_disp: m = 0': 1,
    'dsq_fit_disp: p = 0': 1,
    'dsq_fit_disp: useWeights without weights': 1,
    'dsq_fit_disp: layout = GENE_MAJOR': 1,
    'dsq_fit_disp_rows: NULL args': 1,
    'dsq_fit_disp_rows: NULL out': 1,
    'dsq_fit_disp_rows: args.y NULL': 1,
    'dsq_fit_disp_rows: args.x NULL': 1,
    'dsq_fit_disp_rows: args.mu_hat NULL': 1,
    'dsq_fit_disp_rows: args.log_alpha NULL': 1,
    'dsq_fit_disp_rows: args.log_alpha_prior_mean NULL': 1,
    'dsq_fit_disp_rows: out.log_alpha NULL': 1,
    'dsq_fit_disp_rows: out.last_change NULL': 1,
    'dsq_fit_disp_rows: out.initial_lp NULL': 1,
    'dsq_fit_disp_rows: out.initial_dlp NULL': 1,
    'dsq_fit_disp_rows: out.last_lp NULL': 1,
    'dsq_fit_disp_rows: out.last_dlp NULL': 1,
    'dsq_fit_disp_rows: out.last_d2lp NULL': 1,
    'dsq_fit_disp_rows: out.iter NULL': 1,
    'dsq_fit_disp_rows: out.iter_accept NULL': 1,
    'dsq_fit_disp_rows: n = -1': 1,
    'dsq_fit_disp_rows: m = 0': 1,
    'dsq_fit_disp_rows: p = 0': 1,
    'dsq_fit_disp_rows: useWeights without weights': 1,
    'dsq_fit_disp_rows: layout = GENE_MAJOR': 1,
    'dsq_fit_disp_rows: row range past n': 1,
    'dsq_fit_disp_dev: NULL args': 1,
    'dsq_fit_disp_dev: NULL out': 1,
    'dsq_fit_disp_dev: args.y NULL': 1,
    'dsq_fit_disp_dev: args.x NULL': 1,
    'dsq_fit_disp_dev: args.mu_hat NULL': 1,
    'dsq_fit_disp_dev: args.log_alpha NULL': 1,
    'dsq_fit_disp_dev: args.log_alpha_prior_mean NULL': 1,
    'dsq_fit_disp_dev: out.log_alpha NULL': 1,
    'dsq_fit_disp_dev: out.last_change NULL': 1,
    'dsq_fit_disp_dev: out.initial_lp NULL': 1,
    'dsq_fit_disp_dev: out.initial_dlp NULL': 1,
    'dsq_fit_disp_dev: out.last_lp NULL': 1,
    'dsq_fit_disp_dev: out.last_dlp NULL': 1,
    'dsq_fit_disp_dev: out.iter NULL': 1,
    'dsq_fit_disp_dev: out.iter_accept NULL': 1,
    'dsq_fit_disp_dev: n = -1': 1,
    'dsq_fit_disp_dev: m = 0': 1,
    'dsq_fit_disp_dev: p = 0': 1,
    'dsq_fit_disp_dev: p = 65': 2,
    'dsq_fit_disp_dev: useWeights without weights': 1,
    'dsq_fit_disp_dev: maxit = -1': 1,
    'dsq_fit_disp_dev: gene-major, ld < m': 1,
    'dsq_fit_disp_dev: layout = 7': 1,
    'dsq_fit_disp_grid: NULL args': 1,
    'dsq_fit_disp_grid: NULL out': 1,
    'dsq_fit_disp_grid: args.y NULL': 1,
    'dsq_fit_disp_grid: args.x NULL': 1,
    'dsq_fit_disp_grid: args.mu_hat NULL': 1,
    'dsq_fit_disp_grid: args.disp_grid NULL': 1,
    'dsq_fit_disp_grid: args.log_alpha_prior_mean NULL': 1,
    'dsq_fit_disp_grid: out.log_alpha NULL': 1,
    'dsq_fit_disp_grid: n = -1': 1,
    'dsq_fit_disp_grid: m = 0': 1,
    'dsq_fit_disp_grid: p = 0': 1,
    'dsq_fit_disp_grid: useWeights without weights': 1,
    'dsq_fit_disp_grid: ngrid = 1': 1,
    'dsq_fit_disp_grid: layout = GENE_MAJOR': 1,
    'dsq_fit_disp_grid_rows: NULL args': 1,
    'dsq_fit_disp_grid_rows: NULL out': 1,
    'dsq_fit_disp_grid_rows: args.y NULL': 1,
    'dsq_fit_disp_grid_rows: args.x NULL': 1,
    'dsq_fit_disp_grid_rows: args.mu_hat NULL': 1,
    'dsq_fit_disp_grid_rows: args.disp_grid NULL': 1,
    'dsq_fit_disp_grid_rows: args.log_alpha_prior_mean NULL': 1,
    'dsq_fit_disp_grid_rows: out.log_alpha NULL': 1,
    'dsq_fit_disp_grid_rows: n = -1': 1,
    'dsq_fit_disp_grid_rows: m = 0': 1,
    'dsq_fit_disp_grid_rows: p = 0': 1,
    'dsq_fit_disp_grid_rows: useWeights without weights': 1,
    'dsq_fit_disp_grid_rows: ngrid = 1': 1,
    'dsq_fit_disp_grid_rows: layout = GENE_MAJOR': 1,
    'dsq_fit_disp_grid_rows: row range past n': 1,
    'dsq_fit_disp_grid_dev: NULL args': 1,
    'dsq_fit_disp_grid_dev: NULL out': 1,
    'dsq_fit_disp_grid_dev: args.y NULL': 1,
    'dsq_fit_disp_grid_dev: args.x NULL': 1,
    'dsq_fit_disp_grid_dev: args.mu_hat NULL': 1,
    'dsq_fit_disp_grid_dev: args.disp_grid NULL': 1,
    'dsq_fit_disp_grid_dev: args.log_alpha_prior_mean NULL': 1,
    'dsq_fit_disp_grid_dev: out.log_alpha NULL': 1,
    'dsq_fit_disp_grid_dev: n = -1': 1,
    'dsq_fit_disp_grid_dev: m = 0': 1,
    'dsq_fit_disp_grid_dev: p = 0': 1,
    'dsq_fit_disp_grid_dev: p = 65': 2,
    'dsq_fit_disp_grid_dev: useWeights without weights': 1,
    'dsq_fit_disp_grid_dev: ngrid = 1': 1,
    'dsq_fit_disp_grid_dev: gene-major, ld < m': 1,
    'dsq_fit_disp_grid_dev: layout = 7': 1,
    'dsq_prefit_moments: NULL args': 1,
    'dsq_prefit_moments: NULL out': 1,
    'dsq_prefit_moments: args.y NULL': 1,
    'dsq_prefit_moments: args.nf NULL': 1,
    'dsq_prefit_moments: args.q NULL': 1,
    'dsq_prefit_moments: args.a NULL': 1,
    'dsq_prefit_moments: args.r NULL': 1,
    'dsq_prefit_moments: out.baseMean NULL': 1,
    'dsq_prefit_moments: out.baseVar NULL': 1,
    'dsq_prefit_moments: out.allZero NULL': 1,
    'dsq_prefit_moments: out.roughDisp NULL': 1,
    'dsq_prefit_moments: out.beta_init NULL': 1,
    'dsq_prefit_moments: n = -1': 1,
    'dsq_prefit_moments: m = 0': 1,
    'dsq_prefit_moments: p = 0': 1,
    'dsq_prefit_moments: useWeights without weights': 1,
    'dsq_prefit_moments: layout = GENE_MAJOR': 1,
    'dsq_prefit_moments_dev: NULL args': 1,
    'dsq_prefit_moments_dev: NULL out': 1,
    'dsq_prefit_moments_dev: args.y NULL': 1,
    'dsq_prefit_moments_dev: args.nf NULL': 1,
    'dsq_prefit_moments_dev: args.q NULL': 1,
    'dsq_prefit_moments_dev: args.a NULL': 1,
    'dsq_prefit_moments_dev: args.r NULL': 1,
    'dsq_prefit_moments_dev: out.baseMean NULL': 1,
    'dsq_prefit_moments_dev: out.baseVar NULL': 1,
    'dsq_prefit_moments_dev: out.allZero NULL': 1,
    'dsq_prefit_moments_dev: out.roughDisp NULL': 1,
    'dsq_prefit_moments_dev: out.beta_init NULL': 1,
    'dsq_prefit_moments_dev: n = -1': 1,
    'dsq_prefit_moments_dev: m = 0': 1,
    'dsq_prefit_moments_dev: p = 0': 1,
    'dsq_prefit_moments_dev: p = 65': 1,
    'dsq_prefit_moments_dev: useWeights without weights': 1,
    'dsq_prefit_moments_dev: m <= p': 1,
    'dsq_prefit_moments_dev: gene-major, ld < m': 1,
    'dsq_linear_mu: NULL args': 1,
    'dsq_linear_mu: NULL out': 1,
    'dsq_linear_mu: args.y NULL': 1,
    'dsq_linear_mu: args.nf NULL': 1,
    'dsq_linear_mu: args.q NULL': 1,
    'dsq_linear_mu: args.a NULL': 1,
    'dsq_linear_mu: n = -1': 1,
    'dsq_linear_mu: m = 0': 1,
    'dsq_linear_mu: p = 0': 1,
    'dsq_linear_mu: layout = GENE_MAJOR': 1,
    'dsq_linear_mu_dev: NULL args': 1,
    'dsq_linear_mu_dev: NULL out': 1,
    'dsq_linear_mu_dev: args.y NULL': 1,
    'dsq_linear_mu_dev: args.nf NULL': 1,
    'dsq_linear_mu_dev: args.q NULL': 1,
    'dsq_linear_mu_dev: args.a NULL': 1,
    'dsq_linear_mu_dev: n = -1': 1,
    'dsq_linear_mu_dev: m = 0': 1,
    'dsq_linear_mu_dev: p = 0': 1,
    'dsq_linear_mu_dev: gene-major, ld < m': 1,
    'dsq_nbinom_loglike: NULL args': 1,
    'dsq_nbinom_loglike: NULL out': 1,
    'dsq_nbinom_loglike: args.y NULL': 1,
    'dsq_nbinom_loglike: args.mu NULL': 1,
    'dsq_nbinom_loglike: args.disp NULL': 1,
    'dsq_nbinom_loglike: n = -1': 1,
    'dsq_nbinom_loglike: m = 0': 1,
    'dsq_nbinom_loglike: useWeights without weights': 1,
    'dsq_nbinom_loglike: layout = GENE_MAJOR': 1,
    'dsq_nbinom_loglike_dev: NULL args': 1,
    'dsq_nbinom_loglike_dev: NULL out': 1,
    'dsq_nbinom_loglike_dev: args.y NULL': 1,
    'dsq_nbinom_loglike_dev: args.mu NULL': 1,
    'dsq_nbinom_loglike_dev: args.disp NULL': 1,
    'dsq_nbinom_loglike_dev: n = -1': 1,
    'dsq_nbinom_loglike_dev: m = 0': 1,
    'dsq_nbinom_loglike_dev: useWeights without weights': 1,
    'dsq_nbinom_loglike_dev: gene-major, ld < m': 1,
    'dsq_intercept_fit: NULL args': 1,
    'dsq_intercept_fit: NULL out': 1,
    'dsq_intercept_fit: args.y NULL': 1,
    'dsq_intercept_fit: args.nf NULL': 1,
    'dsq_intercept_fit: args.alpha NULL': 1,
    'dsq_intercept_fit: out.beta_log2 NULL': 1,
    'dsq_intercept_fit: out.betaSE NULL': 1,
    'dsq_intercept_fit: n = -1': 1,
    'dsq_intercept_fit: m = 0': 1,
    'dsq_intercept_fit: useWeights without weights': 1,
    'dsq_intercept_fit: layout = GENE_MAJOR': 1,
    'dsq_intercept_fit_dev: NULL args': 1,
    'dsq_intercept_fit_dev: NULL out': 1,
    'dsq_intercept_fit_dev: args.y NULL': 1,
    'dsq_intercept_fit_dev: args.nf NULL': 1,
    'dsq_intercept_fit_dev: args.alpha NULL': 1,
    'dsq_intercept_fit_dev: out.beta_log2 NULL': 1,
    'dsq_intercept_fit_dev: out.betaSE NULL': 1,
    'dsq_intercept_fit_dev: n = -1': 1,
    'dsq_intercept_fit_dev: m = 0': 1,
    'dsq_intercept_fit_dev: useWeights without weights': 1,
    'dsq_intercept_fit_dev: gene-major, ld < m': 1,
    'dsq_cooks_distance: NULL args': 1,
    'dsq_cooks_distance: NULL out': 1,
    'dsq_cooks_distance: args.y NULL': 1,
    'dsq_cooks_distance: args.nf NULL': 1,
    'dsq_cooks_distance: args.mu NULL': 1,
    'dsq_cooks_distance: args.H NULL': 1,
    'dsq_cooks_distance: args.cell_of NULL': 1,
    'dsq_cooks_distance: out.cooks NULL': 1,
    'dsq_cooks_distance: out.maxCooks NULL': 1,
    'dsq_cooks_distance: n = -1': 1,
    'dsq_cooks_distance: m = 0': 1,
    'dsq_cooks_distance: layout = GENE_MAJOR': 1,
    'dsq_cooks_distance_dev: NULL args': 1,
    'dsq_cooks_distance_dev: NULL out': 1,
    'dsq_cooks_distance_dev: args.y NULL': 1,
    'dsq_cooks_distance_dev: args.nf NULL': 1,
    'dsq_cooks_distance_dev: args.mu NULL': 1,
    'dsq_cooks_distance_dev: args.H NULL': 1,
    'dsq_cooks_distance_dev: args.cell_of NULL': 1,
    'dsq_cooks_distance_dev: out.cooks NULL': 1,
    'dsq_cooks_distance_dev: out.maxCooks NULL': 1,
    'dsq_cooks_distance_dev: n = -1': 1,
    'dsq_cooks_distance_dev: m = 0': 1,
    'dsq_cooks_distance_dev: p = 0': 1,
    'dsq_cooks_distance_dev: ncell = 0': 1,
    'dsq_cooks_distance_dev: gene-major, ld < m': 1,
    'dsq_replace_outliers: NULL args': 1,
    'dsq_replace_outliers: NULL out': 1,
    'dsq_replace_outliers: args.y NULL': 1,
    'dsq_replace_outliers: args.nf NULL': 1,
    'dsq_replace_outliers: args.cooks NULL': 1,
    'dsq_replace_outliers: args.replaceable NULL': 1,
    'dsq_replace_outliers: out.newCounts NULL': 1,
    'dsq_replace_outliers: out.replace NULL': 1,
    'dsq_replace_outliers: n = -1': 1,
    'dsq_replace_outliers: m = 0': 1,
    'dsq_replace_outliers: layout = GENE_MAJOR': 1,
    'dsq_replace_outliers_dev: NULL args': 1,
    'dsq_replace_outliers_dev: NULL out': 1,
    'dsq_replace_outliers_dev: args.y NULL': 1,
    'dsq_replace_outliers_dev: args.nf NULL': 1,
    'dsq_replace_outliers_dev: args.cooks NULL': 1,
    'dsq_replace_outliers_dev: args.replaceable NULL': 1,
    'dsq_replace_outliers_dev: out.newCounts NULL': 1,
    'dsq_replace_outliers_dev: out.replace NULL': 1,
    'dsq_replace_outliers_dev: n = -1': 1,
    'dsq_replace_outliers_dev: m = 0': 1,
    'dsq_replace_outliers_dev: trim = 0.5': 1,
    'dsq_replace_outliers_dev: gene-major, ld < m': 1,
    'dsq_size_factors: NULL args': 1,
    'dsq_size_factors: NULL out': 1,
    'dsq_size_factors: args.y NULL': 1,
    'dsq_size_factors: args.normMatrix NULL': 1,
    'dsq_size_factors: out.sizeFactors NULL': 1,
    'dsq_size_factors: out.normalizationFactors NULL': 1,
    'dsq_size_factors: out.status NULL': 1,
    'dsq_size_factors: n = -1': 1,
    'dsq_size_factors: m = 0': 1,
    'dsq_size_factors: y_type = 7': 1,
    'dsq_size_factors: type = 9': 1,
    'dsq_size_factors: layout = GENE_MAJOR': 1,
    'dsq_size_factors_dev: NULL args': 1,
    'dsq_size_factors_dev: NULL out': 1,
    'dsq_size_factors_dev: args.y NULL': 1,
    'dsq_size_factors_dev: args.normMatrix NULL': 1,
    'dsq_size_factors_dev: out.sizeFactors NULL': 1,
    'dsq_size_factors_dev: out.loggeomeans NULL': 1,
    'dsq_size_factors_dev: out.normalizationFactors NULL': 1,
    'dsq_size_factors_dev: out.status NULL': 1,
    'dsq_size_factors_dev: n = -1': 1,
    'dsq_size_factors_dev: m = 0': 1,
    'dsq_size_factors_dev: y_type = 7': 1,
    'dsq_size_factors_dev: type = 9': 1,
    'dsq_size_factors_dev: gene-major, ld < m': 1,
    'dsq_size_factors_dev: layout = 7': 1,
    'dsq_vst: NULL args': 1,
    'dsq_vst: NULL out': 1,
    'dsq_vst: args.y NULL': 1,
    'dsq_vst: args.nf NULL': 1,
    'dsq_vst: out.rowMean NULL': 1,
    'dsq_vst: out.rowMax NULL': 1,
    'dsq_vst: n = -1': 1,
    'dsq_vst: m = 0': 1,
    'dsq_vst: y_type = 7': 1,
    'dsq_vst: kind = 9': 1,
    'dsq_vst: layout = GENE_MAJOR': 1,
    'dsq_vst_dev: NULL args': 1,
    'dsq_vst_dev: NULL out': 1,
    'dsq_vst_dev: args.y NULL': 1,
    'dsq_vst_dev: args.nf NULL': 1,
    'dsq_vst_dev: out.out NULL': 1,
    'dsq_vst_dev: n = -1': 1,
    'dsq_vst_dev: m = 0': 1,
    'dsq_vst_dev: y_type = 7': 1,
    'dsq_vst_dev: kind = 9': 1,
    'dsq_vst_dev: gene-major, ld < m': 1,
    'dsq_vst_dev: layout = 7': 1,
    'dsq_vst_rowstats_dev: NULL args': 1,
    'dsq_vst_rowstats_dev: NULL out': 1,
    'dsq_vst_rowstats_dev: args.y NULL': 1,
    'dsq_vst_rowstats_dev: args.nf NULL': 1,
    'dsq_vst_rowstats_dev: out.rowMean NULL': 1,
    'dsq_vst_rowstats_dev: out.rowMax NULL': 1,
    'dsq_vst_rowstats_dev: n = -1': 1,
    'dsq_vst_rowstats_dev: m = 0': 1,
    'dsq_vst_rowstats_dev: y_type = 7': 1,
    'dsq_vst_rowstats_dev: gene-major, ld < m': 1,
    'dsq_vst_rowstats_dev: layout = 7': 1,
    'dsq_optim_rows: NULL args': 1,
    'dsq_optim_rows: NULL out': 1,
    'dsq_optim_rows: args.y NULL': 1,
    'dsq_optim_rows: args.x NULL': 1,
    'dsq_optim_rows: args.nf NULL': 1,
    'dsq_optim_rows: args.alpha_hat NULL': 1,
    'dsq_optim_rows: args.lambda NULL': 1,
    'dsq_optim_rows: args.beta_start NULL': 1,
    'dsq_optim_rows: out.beta NULL': 1,
    'dsq_optim_rows: out.betaSE NULL': 1,
    'dsq_optim_rows: out.conv NULL': 1,
    'dsq_optim_rows: out.mu NULL': 1,
    'dsq_optim_rows: out.logLike NULL': 1,
    'dsq_optim_rows: n = -1': 1,
    'dsq_optim_rows: m = 0': 1,
    'dsq_optim_rows: p = 0': 1,
    'dsq_optim_rows: p = 65': 2,
    'dsq_optim_rows: useWeights without weights': 1,
    'dsq_optim_rows: layout = GENE_MAJOR': 1,
    'dsq_parametric_dispersion_fit: first input NULL': 1,
    'dsq_parametric_dispersion_fit: output NULL': 1,
    'dsq_parametric_dispersion_fit: n = -1': 1,
    'dsq_parametric_dispersion_fit_dev: first input NULL': 1,
    'dsq_parametric_dispersion_fit_dev: output NULL': 1,
    'dsq_parametric_dispersion_fit_dev: n = -1': 1,
    'dsq_test_math: first input NULL': 1,
    'dsq_test_math: output NULL': 1,
    'dsq_test_math: n = -1': 1,
    'dsq_parametric_dispersion_fit: n = 0': 1,
    'dsq_parametric_dispersion_fit_dev: n = 0': 1,
    'dsq_test_math: op 7 without b': 1,
}


# What the change itself moved, pinned as it now stands (each decided before the device is looked for).  The host entries run
# the whole check_<call> first, so an EMPTY call (n == 0), which the parent's host half answered with DSQ_OK once a device was
# there, now reports what only its device half refused; and a design that is too wide is reported only when nothing else is wrong.
_CHANGED_CODES = {
    "dsq_fit_beta: n = 0 and p = 65": 2,
    "dsq_fit_beta: n = 0 and maxit = -1": 1,
    "dsq_prefit_moments: n = 0 and m <= p": 1,
    "dsq_optim_rows: p = 65 and layout = GENE_MAJOR": 2,
    "dsq_fit_beta_dev: p = 65 and args.y NULL": 1,
    "dsq_fit_disp_dev: p = 65 and args.log_alpha NULL": 1,
}


# The math hook's ops that read b or c refuse a call without them (the ops from 12 up came with the hook's extension to the
# entry points the kernels call; an op that reads a alone is not listed: it gets past the checks and needs a device).
_MATH_HOOK_CODES = dict([("dsq_test_math: op %d without b" % op, 1) for op in (8, 10, 11, 15, 17, 22)] +
                        [("dsq_test_math: op %d with b, without c" % op, 1) for op in (8, 22)])


def _changed_cases():
    from deseq2_amd import _lib
    from tests import capi_blocks as cb
    B = _tiny_blocks()
    how = {"dsq_fit_beta": (B["fit_beta"], False), "dsq_prefit_moments": (B["prefit_moments"], False),
           "dsq_optim_rows": (B["optim_rows"], False), "dsq_fit_beta_dev": (B["fit_beta"], True),
           "dsq_fit_disp_dev": (B["fit_disp"], True)}
    edits = {"n = 0 and p = 65": dict(n=0, p=65), "n = 0 and maxit = -1": dict(n=0, maxit=-1), "n = 0 and m <= p": dict(n=0, p=6),
             "p = 65 and layout = GENE_MAJOR": dict(p=65, layout=1, ld=8), "p = 65 and args.y NULL": dict(p=65, y=None),
             "p = 65 and args.log_alpha NULL": dict(p=65, log_alpha=None)}
    out = {}
    for cid in _CHANGED_CODES:
        ename, what = cid.split(": ")
        b, dev = how[ename]
        b = b.but(**edits[what])

        def run(b=b, dev=dev, ename=ename):
            a = b.args({k: cb.ptr(None if v is None else cb.fcol(v)) for k, v in b.inputs.items()})
            outs = {k: np.zeros(shape, dtype=dt, order="F") for k, (shape, dt) in b.outputs.items()}
            return cb._invoke(b, getattr(_lib.lib(), ename), a, {k: cb.ptr(v) for k, v in outs.items()}, (None,) if dev else ())
        out[cid] = run
    return out


def test_argument_errors_are_pinned():
    from deseq2_amd import _lib
    L = _lib.lib()
    cases = dict(_argument_cases())
    assert set(_ARGUMENT_CODES) <= set(cases), sorted(set(_ARGUMENT_CODES) - set(cases))
    assert len(_ARGUMENT_CODES) > 200
    cases.update(_changed_cases())
    wrong = []
    assert set(_MATH_HOOK_CODES) <= set(cases)
    for cid, want in {**_ARGUMENT_CODES, **_CHANGED_CODES, **_MATH_HOOK_CODES}.items():
        # dsq_last_error() keeps the last text: leave a known one behind first, so that an entry which fails without
        # writing its own message is seen
        assert L.dsq_test_math(0, None, None, None, None, 0) == 1
        sentinel = L.dsq_last_error()
        assert sentinel == b"bad arguments"
        got = cases[cid]()
        msg = L.dsq_last_error()
        own_text = bool(msg) and (msg != sentinel or cid.startswith(("dsq_parametric_dispersion_fit", "dsq_test_math")))
        if got != want or not own_text:
            wrong.append((cid, want, got, msg))
    assert not wrong, wrong
