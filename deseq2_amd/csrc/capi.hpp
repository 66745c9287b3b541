// capi.hpp -- what the two halves of the C ABI (capi.hip: device pointers, capi_host.hip: host pointers) share.
#pragma once
#include "../../include/deseq2_mi355x.h"
#include "dsq_internal.hpp"

namespace dsq {

static inline void prof_begin(hipStream_t st) { capi_prof_begin("call", 0, st); }
static inline void prof_end(hipStream_t st) { capi_prof_end(st); }

enum {  // workspace slots
    WS_Y = 0, WS_NF, WS_W, WS_MU, WS_HAT, WS_MUOUT, WS_SCRATCH, WS_BAD, WS_CELLS, WS_COOKS_IN, WS_COUNTER, WS_TREND, WS_PAD_X, WS_PAD_VEC, WS_PAD_BETA,
    WS_CELLS_BETA, WS_VST_TABLE, WS_ASH_TABLE,
    // host-entry staging
    WS_H_Y, WS_H_X, WS_H_NF, WS_H_W, WS_H_MU, WS_H_VEC, WS_H_OUTMAT, WS_H_OUTMAT2, WS_H_OUTVEC,
    WS_COUNT
};
static_assert(WS_COUNT <= DSQ_WS_PIPE_PADXR, "pipeline workspace slots follow the call slots");

// unmix(): the threads of a workgroup, i.e. the T of the summation order of DESIGN.md section 17 (thread t adds genes t, t + T, ...)
constexpr int kUnmixThreads = 256;
// estimateSizeFactors(type = "iterate"): the consecutive genes one partial column sum of the gradient covers, i.e. the G of
// the summation order of DESIGN.md section 18
constexpr int kSfIterSliceGenes = 64;

static inline long round_ld(int m) { return ((long)m + 7) & ~7L; }
static inline bool is_wide(int p) { return p > DSQ_P_REG && p <= DSQ_P_WIDE; }
static inline int wide_width(int p) { return dsq_wide_width(p); }   // padded width for a wide p

// capi.hip: layout conversion into the workspace, and the device-pointer bodies behind the entry points (the caller
// holds the call lock and has latched the stream's context)
int prep_counts(const void *y, int y_type, int layout, long ld_in, int n, int m, hipStream_t st,
                const int32_t **out, long *ld_out, bool *checked_async);
int prep_matrix(const double *src, int layout, long ld_in, int n, int m, int slot, hipStream_t st,
                const double **out, long ld_expected);
int finish_ycheck(bool ycheck, hipStream_t st);
// a zero-padded copy of a design in a workspace slot of the latched context: column-major rows x p -> rows x pw (memset,
// then a device-to-device copy of the true columns, on `st`); the calls' wide designs and the chain's three use it
int capi_pad_design(int slot, const double *src, size_t rows, int p, int pw, hipStream_t st, const double **out);
// each call's checks, stated once: everything that can be decided from the argument block alone.  Both halves call it
// first (then: the device, then an empty call returns DSQ_OK); a host entry adds check_host_layout and its row range
int check_fit_beta(const DsqFitBetaArgs *a, const DsqFitBetaOut *o);
int check_fit_disp(const DsqFitDispArgs *a, const DsqFitDispOut *o);
int check_fit_disp_grid(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o);
int check_trend_fit(const double *means, const double *disps, int64_t n, const double *coefs, const int32_t *status);
int check_prefit(const DsqPrefitArgs *a, const DsqPrefitOut *o);
int check_linear_mu(const DsqPrefitArgs *a, const double *mu);
int check_loglike(const DsqLogLikeArgs *a, const double *out);
int check_intercept(const DsqInterceptArgs *a, const DsqInterceptOut *o);
int check_optim(const DsqOptimArgs *a, const DsqOptimOut *o);
int check_cooks(const DsqCooksArgs *a, const DsqCooksOut *o);
int check_replace(const DsqReplaceArgs *a, const DsqReplaceOut *o);
int size_factors_check(const DsqSizeFactorArgs *a, const DsqSizeFactorOut *o);
int vst_check(const DsqVstArgs *a, const DsqVstOut *o, bool transform, bool stats);
int rlog_check(const DsqRlogArgs *a, const DsqRlogOut *o);
int apeglm_check(const DsqApeglmArgs *a, const DsqApeglmOut *o);
int ash_check(const DsqAshArgs *a, const DsqAshOut *o);
int unmix_check(const DsqUnmixArgs *a, const DsqUnmixOut *o);
int sf_iterate_check(const DsqSfIterateArgs *a, const DsqSfIterateOut *o);
int top_var_check(const DsqTopVarArgs *a, const DsqTopVarOut *o);
int sample_pairs_check(const DsqSamplePairsArgs *a, const DsqSamplePairsOut *o);
int collapse_check(const DsqCollapseArgs *a, const DsqCollapseOut *o);
int col_sums_check(const DsqColSumsArgs *a, const DsqColSumsOut *o);
int fpm_check(const DsqFpmArgs *a, const DsqFpmOut *o);
int local_fit_check(const DsqLocalFitArgs *a, const DsqLocalFitOut *o);
int results_check(const DsqResultsArgs *a, const DsqResultsOut *o);
int contrasts_check(const DsqContrastsArgs *a, const DsqContrastsOut *o);
int pt_check(const double *q, const double *df, int32_t n, int32_t K, int32_t tail, const double *out);
int check_host_layout(int layout);
// the device-pointer bodies behind the entry points
int fit_beta_dev_locked(const DsqFitBetaArgs *a, const DsqFitBetaOut *o, hipStream_t st);
int fit_disp_dev_locked(const DsqFitDispArgs *a, const DsqFitDispOut *o, hipStream_t st);
int fit_disp_grid_dev_locked(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o, hipStream_t st);
int prefit_dev_locked(const DsqPrefitArgs *a, const DsqPrefitOut *o, hipStream_t st);
int linear_mu_dev_locked(const DsqPrefitArgs *a, double mu_floor, double *mu, hipStream_t st);
int loglike_dev_locked(const DsqLogLikeArgs *a, double *out, hipStream_t st);
int intercept_dev_locked(const DsqInterceptArgs *a, const DsqInterceptOut *o, hipStream_t st);
int cooks_dev_locked(const DsqCooksArgs *a, const DsqCooksOut *o, hipStream_t st);
int replace_dev_locked(const DsqReplaceArgs *a, const DsqReplaceOut *o, hipStream_t st);
int size_factors_dev_locked(const DsqSizeFactorArgs *a, const DsqSizeFactorOut *o, hipStream_t st);
int vst_dev_locked(const DsqVstArgs *a, const DsqVstOut *o, bool transform, bool stats, hipStream_t st);
int rlog_dev_locked(const DsqRlogArgs *a, const DsqRlogOut *o, hipStream_t st);
int apeglm_dev_locked(const DsqApeglmArgs *a, const DsqApeglmOut *o, hipStream_t st);
int ash_dev_locked(const DsqAshArgs *a, const DsqAshOut *o, void *workspace, int64_t workspace_bytes, hipStream_t st);
int unmix_dev_locked(const DsqUnmixArgs *a, const DsqUnmixOut *o, void *workspace, int64_t workspace_bytes, hipStream_t st);
int sf_iterate_dev_locked(const DsqSfIterateArgs *a, const DsqSfIterateOut *o, void *workspace, int64_t workspace_bytes, hipStream_t st);
int top_var_dev_locked(const DsqTopVarArgs *a, const DsqTopVarOut *o, hipStream_t st);
int sample_pairs_dev_locked(const DsqSamplePairsArgs *a, const DsqSamplePairsOut *o, hipStream_t st);
int collapse_dev_locked(const DsqCollapseArgs *a, const DsqCollapseOut *o, hipStream_t st);
int col_sums_dev_locked(const DsqColSumsArgs *a, const DsqColSumsOut *o, hipStream_t st);
int fpm_dev_locked(const DsqFpmArgs *a, const DsqFpmOut *o, hipStream_t st);
int local_fit_dev_locked(const DsqLocalFitArgs *a, const DsqLocalFitOut *o, hipStream_t st);
int results_dev_locked(const DsqResultsArgs *a, const DsqResultsOut *o, hipStream_t st);
int contrasts_dev_locked(const DsqContrastsArgs *a, const DsqContrastsOut *o, hipStream_t st);

}  // namespace dsq
