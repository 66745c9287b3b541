"""ctypes binding of libdeseq2_mi355x.so.

include/deseq2_mi355x.h is the one statement of the ABI; this module mirrors it -- the constants, the argument and output
blocks, and ONE table of signatures that lib() applies -- and tests/test_capi_cpu.py holds every line of the mirror to the
header as the C compiler reads it.

The shared library is built in-tree by `__graft_entry__.build()` (or
`make -C deseq2_amd/csrc`).  There is no fallback: if the library is missing or no
gfx950 device is usable, calls raise.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("DSQ_LIB") or os.path.join(_HERE, "libdeseq2_mi355x.so")   # DSQ_LIB: tuning builds only

# ---- constants ---------------------------------------------------------------------------------------------------------
DSQ_OK = 0
DSQ_ERR_ARG, DSQ_ERR_UNSUPPORTED, DSQ_ERR_DEVICE, DSQ_ERR_NOMEM, DSQ_ERR_VALUE, DSQ_ERR_FIT = 1, 2, 3, 4, 5, 6
ERR_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("DSQ_ERR_")}
DSQ_LAYOUT_R, DSQ_LAYOUT_GENE_MAJOR = 0, 1
DSQ_Y_INT32, DSQ_Y_FLOAT64 = 0, 1
DSQ_MAX_P = 64
DSQ_RESULTS_MAX_K = 4096
DSQ_VST_MAX_KNOTS = 1600
DSQ_UNMIX_MAX_K = 16
DSQ_APEGLM_MAX_P = 16
DSQ_ASH_MAX_K = 64
DSQ_PH_GENE_EST, DSQ_PH_TREND, DSQ_PH_MAP_TEST, DSQ_PH_OUTLIERS, DSQ_PH_FINISH, DSQ_PH_PRIOR = 1, 2, 4, 8, 16, 32
DSQ_PH_OUTLIERS_DETECT, DSQ_PH_OUTLIERS_REFIT = 64, 128
DSQ_SC_COEF0, DSQ_SC_COEF1, DSQ_SC_VAR_LOG_DISP, DSQ_SC_DISP_PRIOR_VAR, DSQ_SC_FIT_USED = 0, 1, 2, 3, 4
DSQ_ST_COUNT, DSQ_SC_COUNT = 16, 8
# families keyed by the R-side spelling: key k of DSQ_X is the header's DSQ_X_<K>, K = k in upper case with its camel humps
# split (greaterAbs2014 -> GREATER_ABS_2014); DSQ_FPM alone holds DSQ_FPM, DSQ_FPKM_BASEPAIRS, DSQ_FPKM_TXLEN
DSQ_TEST = {"Wald": 0, "LRT": 1}
DSQ_ALT = {"greaterAbs": 0, "lessAbs": 1, "greater": 2, "less": 3, "greaterAbs2014": 4}
DSQ_PT = {"lower": 0, "upper": 1, "two_sided": 2}
DSQ_VST = {"parametric": 0, "mean": 1, "spline": 2, "log2": 3, "normalized": 4}
DSQ_SF = {"ratio": 0, "poscounts": 1}
DSQ_PAIRS = {"dist2": 0, "dist": 1, "gram": 2}
DSQ_FPM = {"fpm": 0, "fpkm_basepairs": 1, "fpkm_txlen": 2}
DSQ_FIT = {"parametric": 0, "mean": 1, "parametric_or_mean": 2, "given": 3}
DSQ_ST = {k: i for i, k in enumerate((     # the header's enum, in its order
    "N_NONZERO", "N_GRID_GENEEST", "N_TREND", "TREND_STATUS", "N_ABOVE_MIN", "N_GRID_MAP", "N_OPTIM_GENEEST",
    "N_OPTIM_TEST", "N_REPLACE", "N_REFIT", "N_GRID_GENEEST_REFIT", "N_GRID_MAP_REFIT", "N_OPTIM_GENEEST_REFIT",
    "N_OPTIM_TEST_REFIT"))}


class DsqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "DSQ_ERR"), code, msg))
        self.code = code


# ---- argument and output blocks ------------------------------------------------------------------------------------------
_CTYPE = {"i": C.c_int32, "u": C.c_uint32, "l": C.c_int64, "d": C.c_double, "p": C.c_void_p}


def _struct(name, fields):
    """The C.Structure of a block of the header, its fields in the header's order: groups `<type> name name ...` joined by
    `;`, the type one of i (int32_t), u (uint32_t), l (int64_t), d (double), p (any pointer); `name[k]` is an array of k.
    The header's `lambda` is `lambda_` here."""
    fs = []
    for group in fields.split(";"):
        t, *names = group.split()
        for nm, dim in (re.fullmatch(r"(\w+)(?:\[(\d+)\])?", f).groups() for f in names):
            fs.append((nm, _CTYPE[t] * int(dim) if dim else _CTYPE[t]))
    return type(name, (C.Structure,), {"_fields_": fs})


_COUNTS = "i n m layout; l ld; p y; i y_type"          # the count matrix of the entries without a design
_DESIGN = "i n m p layout; l ld; p y; i y_type"        # ... and of those with one
_CELLS = "p cell_of; i ncell"

DsqFitBetaArgs = _struct("DsqFitBetaArgs", _DESIGN + "; p x nf; i nf_is_vector; p alpha_hat contrast beta_mat lambda_ weights;"
                         " i useWeights; d tol; i maxit useQR; d minmu;" + _CELLS)
DsqFitBetaOut = _struct("DsqFitBetaOut", "p beta_mat beta_var_mat iter hat_diagonals contrast_num contrast_denom deviance mu;"
                        " d mu_floor")
DsqFitDispArgs = _struct("DsqFitDispArgs", _DESIGN + "; p x mu_hat log_alpha log_alpha_prior_mean;"
                         " d log_alpha_prior_sigmasq min_log_alpha kappa_0 tol; i maxit usePrior; p weights; i useWeights;"
                         " d weightThreshold; i useCR;" + _CELLS)
DsqFitDispOut = _struct("DsqFitDispOut", "p log_alpha iter iter_accept last_change initial_lp initial_dlp last_lp last_dlp"
                        " last_d2lp")
DsqFitDispGridArgs = _struct("DsqFitDispGridArgs", _DESIGN + "; p x mu_hat disp_grid; i ngrid; p log_alpha_prior_mean;"
                             " d log_alpha_prior_sigmasq; i usePrior; p weights; i useWeights; d weightThreshold; i useCR;"
                             + _CELLS)
DsqFitDispGridOut = _struct("DsqFitDispGridOut", "p log_alpha")
DsqPrefitArgs = _struct("DsqPrefitArgs", _DESIGN + "; p nf; i nf_is_vector; p weights; i useWeights; p q a r")
DsqPrefitOut = _struct("DsqPrefitOut", "p baseMean baseVar allZero roughDisp beta_init")
DsqLogLikeArgs = _struct("DsqLogLikeArgs", _COUNTS + "; p mu disp weights; i useWeights")
DsqInterceptArgs = _struct("DsqInterceptArgs", _COUNTS + "; p nf; i nf_is_vector; p weights; i useWeights; p alpha;"
                           " d mu_floor")
DsqInterceptOut = _struct("DsqInterceptOut", "p beta_log2 betaSE mu hat")
DsqOptimArgs = _struct("DsqOptimArgs", _DESIGN + "; p x nf; i nf_is_vector; p alpha_hat lambda_ weights; i useWeights;"
                       " p beta_start; d minmu")
DsqOptimOut = _struct("DsqOptimOut", "p beta betaSE conv mu logLike")
DsqCooksArgs = _struct("DsqCooksArgs", _DESIGN + "; p nf; i nf_is_vector; p mu H;" + _CELLS)
DsqCooksOut = _struct("DsqCooksOut", "p cooks maxCooks robustDisp")
DsqReplaceArgs = _struct("DsqReplaceArgs", _COUNTS + "; p nf; i nf_is_vector; p cooks; d cooksCutoff trim; p replaceable")
DsqReplaceOut = _struct("DsqReplaceOut", "p newCounts replace")
DsqDeseqArgs = _struct(
    "DsqDeseqArgs", "i n m p; l ld; i phases; p y nf; i nf_is_vector useWeights;"
    " p weights_raw weights_norm weights_floor force_zero x q a r; d xim; i linearMu;"
    " d minDisp kappa_0 dispTol weightThreshold outlierSD betaTol minmu; i maxit useCR useQR betaMaxit; p disp_grid; i ngrid;"
    " d expVarLogDisp; p trend_mean trend_disp; i n_trend; p lambda_; d min_log_alpha; p workspace; l workspace_bytes; i test;"
    + _CELLS + "; p replaceable; d cooksCutoff trim; i do_replace; p x_red q_red a_red r_red; i p_red; p cell_of_red;"
    " i ncell_red defer_finish; p n_refit_global; i betaPrior; p x_prior; i p_prior prior_expanded prior_intercept;"
    " p lambda_prior; i fitType; p dispFit_in trend_fit_in; d dispPriorVar_in")
_MCOLS = ("p baseMean baseVar allZero dispGeneEst dispGeneIter dispFit dispMAP dispersion dispIter dispOutlier beta betaSE stat"
          " pvalue betaConv betaIter logLike logLikeReduced maxCooks replace ")     # the per-gene columns both chains return
DsqDeseqOut = _struct("DsqDeseqOut", _MCOLS + "optim_geneest optim_test mu_hat mu H cooks replaceCounts status scalars mle_beta")
DsqDeseqHostArgs = _struct(
    "DsqDeseqHostArgs", "i n m p; p counts; i y_type; p x sizeFactors normalizationFactors weights q r xrinv; i test;"
    " p x_reduced q_reduced r_reduced; i p_reduced; d minReplicatesForReplace cooksCutoff expVarLogDisp betaTol minmu;"
    " i maxit useQR disp_maxit useCR; p disp_grid; i ngrid betaPrior; p x_prior; i p_prior;"
    " p coef_factor prior_coef_factor prior_coef_src betaPriorVar; i fitType; p dispFit; i geneEstOnly; d dispPriorVar")
DsqDeseqHostOut = _struct("DsqDeseqHostOut", _MCOLS + "weightsFail mu H cooks replaceCounts; d dispersionFunction[8];"
                          " i status[16]; d betaPriorVar[%d]; p mle_beta" % DSQ_MAX_P)
DsqBetaPriorArgs = _struct("DsqBetaPriorArgs", "i n p; p mle_beta baseMean dispFit allZero coef_factor; i expanded p_prior;"
                           " p prior_coef_factor prior_coef_src; d upperQuantile")
DsqSizeFactorArgs = _struct("DsqSizeFactorArgs", _COUNTS + " type; p geoMeans control normMatrix workspace;"
                            " l workspace_bytes")
DsqSizeFactorOut = _struct("DsqSizeFactorOut", "p sizeFactors loggeomeans normalizationFactors status")
DsqVstArgs = _struct("DsqVstArgs", _COUNTS + "; p nf; i nf_is_vector kind; d asymptDisp extraPois alpha pc; p spline;"
                     " i nknots; d eta xi")
DsqVstOut = _struct("DsqVstOut", "p out rowMean rowMax bad")
DsqRlogArgs = _struct("DsqRlogArgs", _COUNTS + "; p nf; i nf_is_vector; p dispFit; d betaPriorVar; p intercept; d tol minmu;"
                      " i maxit")
DsqRlogOut = _struct("DsqRlogOut", "p rlog intercept iter flag bad")
DsqApeglmArgs = _struct("DsqApeglmArgs", _DESIGN + "; p nf; i nf_is_vector; p x weights disp init; i coef; u no_shrink;"
                        " d prior_scale prior_df no_shrink_scale; i has_threshold; d threshold tol; i maxit")
DsqApeglmOut = _struct("DsqApeglmOut", "p map sd fsr thresh iter conv start objective bad")
DsqAshArgs = _struct("DsqAshArgs", "i n C; l ld; p betahat sebetahat; i has_threshold; d threshold; i maxit")
DsqAshOut = _struct("DsqAshOut", "p PosteriorMean PosteriorSD NegativeProb PositiveProb lfsr le_T gt_mT pi sd K iter flag loglik")
DsqUnmixArgs = _struct("DsqUnmixArgs", "i n m k; l ld; p x pure; i has_alpha has_shift; d alpha shift; i power maxit")
DsqUnmixOut = _struct("DsqUnmixOut", "p p loss iter flag")
DsqSfIterateArgs = _struct("DsqSfIterateArgs", "i n m; l ld; p y mu sf disp rows; d Q; i maxit")
DsqSfIterateOut = _struct("DsqSfIterateOut", "p s sf F iter evals flag")
DsqTopVarArgs = _struct("DsqTopVarArgs", "u struct_size; i n m; l ld; p x; i ntop")
DsqTopVarOut = _struct("DsqTopVarOut", "u struct_size; p rowMean rowVar select")
DsqSamplePairsArgs = _struct("DsqSamplePairsArgs", "u struct_size; i n m; l ld; p x; i kind nrows; p rows centre")
DsqSamplePairsOut = _struct("DsqSamplePairsOut", "u struct_size; p out")
DsqCollapseArgs = _struct("DsqCollapseArgs", "u struct_size; i n m g; l ld; p y members offsets")
DsqCollapseOut = _struct("DsqCollapseOut", "u struct_size; l ld; p out status")
DsqColSumsArgs = _struct("DsqColSumsArgs", "u struct_size; i n m; l ld; p y")
DsqColSumsOut = _struct("DsqColSumsOut", "u struct_size; p sums")
DsqFpmArgs = _struct("DsqFpmArgs", "u struct_size; i n m; l ld; p y; i kind; p lib basepairs txlen")
DsqFpmOut = _struct("DsqFpmOut", "u struct_size; p out")
DsqLocalFitArgs = _struct("DsqLocalFitArgs", "u struct_size; i n; p means disps; d minDisp; p fit_in; i n_eval; p eval_means")
DsqLocalFitOut = _struct("DsqLocalFitOut", "u struct_size; p fit dispFit status")
DsqResultsArgs = _struct("DsqResultsArgs", "i n p c test; p beta betaSE stat pvalue baseMean replace na_mask; d lfcThreshold;"
                         " i altHypothesis independentFiltering; p filter theta; i K; d alpha; p workspace; l workspace_bytes;"
                         " p df")
DsqResultsOut = _struct("DsqResultsOut", "p baseMean log2FoldChange lfcSE stat pvalue filtPadj numRej cutoffs status")
DsqContrastsArgs = _struct("DsqContrastsArgs", "i n m p K; l ld; p x nf; i nf_is_vector; p alpha_hat beta lambda_ weights;"
                           " i useWeights; d minmu; p contrasts allZero counts sample_mask rule_applies;" + _CELLS + "; p df")
DsqContrastsOut = _struct("DsqContrastsOut", "p log2FoldChange lfcSE stat pvalue contrastAllZero")


def sized(cls, **kw):
    """an argument block that carries its own size in struct_size"""
    return cls(struct_size=C.sizeof(cls), **kw)


# ---- signatures: symbol -> (restype, argtypes), every function the header declares --------------------------------------
_I, _I32, _I64, _D, _P = C.c_int, C.c_int32, C.c_int64, C.c_double, C.c_void_p
SIGNATURES = {}


def _sig(name, *argtypes, res=_I):
    SIGNATURES[name] = (res, list(argtypes))


def _blocks(args, out):
    return C.POINTER(args), C.POINTER(out)


def _pair(name, *argtypes):
    """a host entry and its _dev twin: the same arguments, then the stream"""
    _sig(name, *argtypes)
    _sig(name + "_dev", *argtypes, _P)


def _workspace_bytes(name, sizes):
    _sig(name + "_workspace_bytes", *[_I32] * sizes, res=_I64)


for _name, _a, _o in (("dsq_fit_beta", DsqFitBetaArgs, DsqFitBetaOut), ("dsq_fit_disp", DsqFitDispArgs, DsqFitDispOut),
                      ("dsq_fit_disp_grid", DsqFitDispGridArgs, DsqFitDispGridOut)):
    _pair(_name, *_blocks(_a, _o))
    _sig(_name + "_rows", *_blocks(_a, _o), _I64, _I64)          # row_lo, row_cnt
for _name, _a, _o in (("dsq_prefit_moments", DsqPrefitArgs, DsqPrefitOut), ("dsq_intercept_fit", DsqInterceptArgs, DsqInterceptOut),
                      ("dsq_cooks_distance", DsqCooksArgs, DsqCooksOut), ("dsq_replace_outliers", DsqReplaceArgs, DsqReplaceOut),
                      ("dsq_size_factors", DsqSizeFactorArgs, DsqSizeFactorOut), ("dsq_vst", DsqVstArgs, DsqVstOut),
                      ("dsq_rlog", DsqRlogArgs, DsqRlogOut), ("dsq_apeglm", DsqApeglmArgs, DsqApeglmOut),
                      ("dsq_top_var", DsqTopVarArgs, DsqTopVarOut),
                      ("dsq_sample_pairs", DsqSamplePairsArgs, DsqSamplePairsOut), ("dsq_collapse", DsqCollapseArgs, DsqCollapseOut),
                      ("dsq_col_sums", DsqColSumsArgs, DsqColSumsOut), ("dsq_fpm", DsqFpmArgs, DsqFpmOut),
                      ("dsq_local_fit", DsqLocalFitArgs, DsqLocalFitOut),
                      ("dsq_results", DsqResultsArgs, DsqResultsOut), ("dsq_contrasts", DsqContrastsArgs, DsqContrastsOut)):
    _pair(_name, *_blocks(_a, _o))
_pair("dsq_nbinom_loglike", C.POINTER(DsqLogLikeArgs), _P)
_pair("dsq_linear_mu", C.POINTER(DsqPrefitArgs), _D, _P)
_pair("dsq_parametric_dispersion_fit", _P, _P, _I64, _P, _P)     # means, disps, n, coefs, status
_pair("dsq_pt", _P, _P, _I32, _I32, _I32, _P, _P)                # q, df, n, K, tail, keep, out
# ... whose device entry also takes the caller's workspace and its size
for _name, _a, _o in (("dsq_unmix", DsqUnmixArgs, DsqUnmixOut), ("dsq_sf_iterate", DsqSfIterateArgs, DsqSfIterateOut),
                      ("dsq_ash", DsqAshArgs, DsqAshOut)):
    _sig(_name, *_blocks(_a, _o))
    _sig(_name + "_dev", *_blocks(_a, _o), _P, _I64, _P)
_sig("dsq_beta_prior_var", C.POINTER(DsqBetaPriorArgs), _P)
_sig("dsq_beta_prior_var_dev", C.POINTER(DsqBetaPriorArgs), _P, _P, _I64, _P)
_sig("dsq_beta_prior_var_columns", C.POINTER(DsqBetaPriorArgs), res=_I32)
_sig("dsq_optim_rows", *_blocks(DsqOptimArgs, DsqOptimOut))
_sig("dsq_vst_rowstats_dev", *_blocks(DsqVstArgs, DsqVstOut), _P)
_sig("dsq_deseq", *_blocks(DsqDeseqHostArgs, DsqDeseqHostOut))
_sig("dsq_deseq_dev", *_blocks(DsqDeseqArgs, DsqDeseqOut), _P)
_workspace_bytes("dsq_deseq", 4)             # n, m, p, n_trend
_workspace_bytes("dsq_size_factors", 2)      # n, m
_workspace_bytes("dsq_unmix", 3)             # n, m, k
_workspace_bytes("dsq_sf_iterate", 2)        # n, m
_workspace_bytes("dsq_results", 2)           # n, K
_workspace_bytes("dsq_ash", 2)               # n, C
_workspace_bytes("dsq_beta_prior_var", 2)    # n, columns
_sig("dsq_weights_prep_dev", _P, _P, _I32, _I32, _I32, _I64, _D, _P, _P, _P, _P, _P)
_sig("dsq_xim_dev", _P, _I32, _I32, _I64, _P, _P, _P)
for _name in ("dsq_to_gene_major_f64", "dsq_to_gene_major_i32", "dsq_from_gene_major_f64"):
    _sig(_name, _P, _P, _I32, _I32, _I64, _P)                    # src, dst, n, m, ld, stream
_sig("dsq_counts_f64_to_gene_major_i32", _P, _P, _I32, _I32, _I64, _P, _P)
_sig("dsq_test_math", _I, _P, _P, _P, _P, _I64)
for _name in ("dsq_unmix_block_threads", "dsq_sf_iterate_slice_genes", "dsq_row_vars_register_width", "dsq_local_fit_lanes",
              "dsq_apeglm_lds_doubles", "dsq_ash_slice_rows"):
    _sig(_name, res=_I32)
_sig("dsq_local_fit_block_doubles", _I32, res=_I64)
_sig("dsq_sample_pairs_slice_rows", _I64, _I32, res=_I64)
_sig("dsq_contrasts_max_m", _I32, res=_I32)
for _name in ("dsq_version", "dsq_device_count", "dsq_release_workspace", "dsq_profile_count"):
    _sig(_name)
_sig("dsq_last_error", res=C.c_char_p)
_sig("dsq_set_device", _I)
_sig("dsq_profile_enable", _I)
_sig("dsq_profile_last_ms", res=_D)
_sig("dsq_profile_get", _I, C.c_char_p, _I, _P, _P)              # i, name, cap, genes, ms

EXPORTED_SYMBOLS = list(SIGNATURES)

_lib = None


def lib():
    """Load libdeseq2_mi355x.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise FileNotFoundError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C deseq2_amd/csrc`.  deseq2_amd has no CPU fallback." % SO_PATH)
    # torch bundles its own HIP/HSA runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).
    # A process must not end up with two runtimes, so when torch is installed it is imported
    # first: the engine library then binds to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != DSQ_OK:
        raise DsqError(rc, lib().dsq_last_error().decode("utf-8", "replace"))
