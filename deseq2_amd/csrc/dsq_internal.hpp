// dsq_internal.hpp -- launch-level parameter blocks shared by the kernels and the C ABI.
// All pointers are device pointers; n x m matrices are gene-major with leading dim ld.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <mutex>
#include <string.h>

namespace dsq {

struct DispKernelParams {
    int n, m, p;
    long ld;
    const int32_t *y;
    const double *mu_hat;
    const double *weights;  // nullptr unless useWeights
    const double *x;        // m x p column-major
    const double *log_alpha_in;
    const double *prior_mean;
    double prior_sigmasq, min_log_alpha, kappa_0, tol, weightThreshold;
    int maxit, usePrior, useWeights, useCR;
    // fitDisp outputs
    double *log_alpha;
    int32_t *iter, *iter_accept;
    double *last_change, *initial_lp, *initial_dlp, *last_lp, *last_dlp, *last_d2lp;
    // fitDispGrid
    const double *grid;
    int ngrid;
    int ablate, force_iters; // profiling only
    int predict;             // evaluator policy of the line search (Tuning::disp_predict) -- set by the launch (fit_disp.hip)
    int xlds;                // 1: X staged in LDS, 0: read through L1/L2
    int *work_counter;       // zeroed int: waves draw their next gene from it (nullptr: static grid-stride)
    unsigned long long padmask;   // WIDE kernels: bit c set = design column c is zero padding
    const double *prior_sigmasq_dev;   // non-null: the prior variance is read from the device (fused pipeline)
    // design cells (see BetaKernelParams): ncell > 0 -> the Cox-Reid matrices are assembled from per-cell sums
    const int32_t *cell_perm, *cell_start;
    int ncell;
    // fused pipeline (pipeline.hip): the launch covers the genes rows[0 .. *n_dev) of full-size arrays (rows == nullptr:
    // genes 0 .. n-1); n stays the capacity / leading dimension of the n-vectors and n x p matrices
    const int32_t *rows;
    const int32_t *n_dev;
    int rows_few;            // the list is expected to be short (stragglers, refits): a one-block-per-CU grid is enough
    // unstaged rows (long rows read through L2), no weights: the distinct-count buffers of the resident waves (2 m int32
    // each) in GLOBAL memory -- set by the launch (fit_disp.hip); the kernel instantiation decides at compile time
    int32_t *dist_global;
};

struct BetaKernelParams {
    int n, m, p;
    long ld;
    const int32_t *y;
    const double *nf;       // gene-major matrix, or m-vector when nf_is_vector
    int nf_is_vector;
    const double *weights;  // nullptr unless useWeights
    const double *x;        // m x p column-major
    const double *alpha_hat;
    const double *contrast;
    const double *beta_init;  // n x p column-major
    const double *lambda;
    double tol, minmu, mu_floor;
    int maxit, useQR, useWeights;
    double *beta_mat, *beta_var_mat, *iter, *hat_diagonals, *contrast_num, *contrast_denom, *deviance;
    double *mu_out;
    double *scratch;        // global per-wave-slot scratch when rows are not staged in LDS
    double *cscratch;       // (unused since the closed-form deviance; kept so that the launch plumbing stays put)
    int ablate, force_iters; // profiling only (env DSQ_ABLATE / DSQ_FORCE_ITERS): skip phases / fixed trip count
    int xlds;                // 1: X staged in LDS, 0: read through L1/L2
    int *work_counter;       // zeroed int: waves draw their next gene from it (nullptr: static grid-stride)
    // fused pipeline (pipeline.hip): the launch covers the genes rows[0 .. *n_dev) of full-size arrays (rows == nullptr:
    // genes 0 .. n-1); n stays the capacity / leading dimension of the n-vectors and n x p matrices
    const int32_t *rows;
    const int32_t *n_dev;
    int rows_few;            // the list is expected to be short (stragglers, refits): a one-block-per-CU grid is enough
    // design cells (samples with identical design rows, numbered by first appearance): ncell > 0 selects the
    // cell-collapsed kernel; cell_perm = samples grouped by cell (ascending inside a cell), cell_start = ncell + 1 offsets
    const int32_t *cell_perm, *cell_start;
    int ncell;
    double *kconst_out;     // n values or NULL: K' of the row -- the mu-independent part of sum [wts] log NB(y; 1/alpha, mu) on
                            // the closed split (dsq_math.hpp) -- for the nbinomLogLike launch that follows this fit
    int p_true;             // WIDE designs: the design's own number of columns (the zero padding follows them); 0 = p.  The
                            // rolled kernel runs at this width -- the padded coefficients' ridge rows and zero columns only
                            // ever add exact zeros to the real ones' sums -- and writes the padding's outputs (0) itself
    // cell kernel only, with hat_diagonals and mu_out: n flags or NULL -- 1 where some sample's Cook's distance can exceed
    // cand_cutoff whatever robust dispersion cooks_kernel finds for the row (the bound next to the kernel's output loops);
    // cand_p: the divisor of the distance, the design's own number of columns
    int32_t *cand_flag;
    double cand_cutoff, cand_p;
};

struct PrefitKernelParams {
    int n, m, p;
    long ld;
    const int32_t *y;
    const double *nf;
    int nf_is_vector;
    const double *weights;
    int useWeights;
    const double *q, *a, *r;   // Q (m x p), X R^-1 (m x p), R (p x p), all column-major
    double *baseMean, *baseVar, *roughDisp, *beta_init;
    int32_t *allZero;
    // fused pipeline (pipeline.hip): the launch covers the genes rows[0 .. *n_dev) of full-size arrays (rows == nullptr:
    // genes 0 .. n-1); n stays the capacity / leading dimension of the n-vectors and n x p matrices
    const int32_t *rows;
    const int32_t *n_dev;
};

struct LogLikeKernelParams {
    int n, m;
    long ld;
    const int32_t *y;
    const double *mu;
    const double *disp;
    const double *weights;
    int useWeights;
    double *loglike;
    // fused pipeline (pipeline.hip): the launch covers the genes rows[0 .. *n_dev) of full-size arrays (rows == nullptr:
    // genes 0 .. n-1); n stays the capacity / leading dimension of the n-vectors and n x p matrices
    const int32_t *rows;
    const int32_t *n_dev;
    const int32_t *skip;     // n flags or NULL: genes with a non-zero flag are left alone (neither read nor written)
    const double *kconst;    // n values or NULL: the mu-independent part of each row's sum, from the fitBeta launch that
                             // fitted the row with the SAME dispersions / weights (BetaKernelParams.kconst_out); NULL: computed here
};

struct InterceptKernelParams {
    int n, m;
    long ld;
    const int32_t *y;
    const double *nf;
    int nf_is_vector;
    const double *weights;
    int useWeights;
    const double *alpha;
    double mu_floor;
    double *beta_log2, *betaSE, *mu_out, *hat;
    double *loglike;         // optional: nbinomLogLike at the (unfloored) fitted means, as loglike_kernel computes it
    // fused pipeline (pipeline.hip): the launch covers the genes rows[0 .. *n_dev) of full-size arrays (rows == nullptr:
    // genes 0 .. n-1); n stays the capacity / leading dimension of the n-vectors and n x p matrices
    const int32_t *rows;
    const int32_t *n_dev;
    const double *kconst;    // as LogLikeKernelParams.kconst (the full model's fit has the same counts, dispersions, weights)
};

struct OptimKernelParams {
    int n, m, p;
    long ld;
    const int32_t *y;
    const double *nf;
    int nf_is_vector;
    const double *weights;
    int useWeights;
    const double *x;           // m x p column-major
    const double *alpha_hat;   // n
    const double *lamnat;      // p: prior precisions on the natural-log scale
    const double *beta_start;  // n x p column-major, log2 scale
    double minmu;
    double *beta, *betaSE;     // n x p column-major, log2 scale
    int32_t *conv;             // n
    double *mu_out;            // n x ld
    double *loglike;           // n
    double mu_floor;           // > 0: the fitted means are stored floored at it (fitMu[fitMu < minmu] <- minmu, R/core.R:763)
    // fused pipeline (pipeline.hip): the launch covers the rows rows[0 .. *n_dev) of full-size arrays (n = their
    // capacity / leading dimension); rows == nullptr: rows 0 .. n-1
    const int32_t *rows;
    const int32_t *n_dev;
};

struct CooksKernelParams {
    int n, m, p;
    long ld;
    const int32_t *y;
    const double *nf;
    int nf_is_vector;
    const double *mu, *H;        // gene-major
    const int32_t *perm;         // sample indices grouped by design cell
    const int32_t *cell_start;   // ncell + 1 offsets into perm
    const int32_t *in3;          // m flags: sample sits in a cell with >= 3 members
    int ncell, any3;
    int sortcap;                 // doubles of sort buffer per wave (power of two)
    double *cooks, *maxCooks, *robustDisp;
    const int32_t *rows;         // fused pipeline: see DispKernelParams
    const int32_t *n_dev;
    const int32_t *skip;         // n flags or NULL: as LogLikeKernelParams.skip
    int rows_few;                // the list is expected to be short: one block per CU is enough
    int beside;                  // the launch runs BESIDE another stream's small launches: it leaves them part of every CU
};

struct ReplaceKernelParams {
    int n, m;
    long ld;
    const int32_t *y;
    const double *nf;
    int nf_is_vector;
    const double *cooks;
    double cutoff, trim;
    const int32_t *replaceable;  // m flags
    int sortcap;
    int32_t *newCounts, *replace;
    const int32_t *rows;
    const int32_t *n_dev;
    const int32_t *skip;         // as CooksKernelParams
    int rows_few, beside;
};

// estimateSizeFactors (size_factors.hip).  Element (i, j) of the counts sits at y[i * y_si + j * y_sj] (either layout), of
// normMatrix / the normalization factors at [i * nm_si + j * nm_sj].  The second block is carved from the caller's
// workspace by launch_size_factors.
struct SizeFactorKernelParams {
    int n, m;
    const void *y;
    long y_si, y_sj;
    const double *nm;            // normMatrix or nullptr
    long nm_si, nm_sj;
    const double *geoMeans;      // n or nullptr
    const int32_t *control;      // n flags or nullptr
    int type;                    // 0 ratio, 1 poscounts
    int stabilize;               // divide by exp(mean(log sf)) (R/core.R:573-576)
    double *sf;                  // m
    double *lgm_out;             // n or nullptr
    double *nf_out;              // normalization factors or nullptr
    int32_t *status;
    double *lgm, *logsf;
    unsigned long long *prefix, *hikey, *hiprefix;
    unsigned int *hist, *cnt, *rank, *histate, *hishift;
    int *any_not_inf;
};
hipError_t launch_size_factors(SizeFactorKernelParams kp, int y_f64, void *workspace, hipStream_t st);
size_t size_factors_workspace_bytes(long n, long m);

// the variance stabilizing transformation (vst.hip).  Element (i, j) of counts / nf matrix / output sits at
// [i * si + j * sj] (either layout; all three share the strides).  kind = DSQ_VST_* of the public header.
struct VstKernelParams {
    int n, m;
    const void *y;
    long si, sj;
    const double *nf;            // m-vector (nf_is_vector) or matrix
    int nf_is_vector;
    int kind;
    double a, e;                 // parametric: asymptDisp, extraPois
    double alpha;                // mean
    double pc;                   // log2
    const double *table;         // spline: DEVICE copy of x | y | b | c | d
    int nknots;
    double eta, xi;
    double *out;
    double *rowMean, *rowMax;
    int32_t *bad;                // float64 counts: set to 1 on a negative / non-finite / non-integer value; may be nullptr
};
hipError_t launch_vst_transform(const VstKernelParams &kp, int y_f64, hipStream_t st);
hipError_t launch_vst_rowstats(const VstKernelParams &kp, int y_f64, hipStream_t st);

// the rlog fit (rlog.hip).  Element (i, j) of counts / nf matrix / output sits at [i * si + j * sj].
struct RlogKernelParams {
    int n, m;
    const void *y;
    long si, sj;
    const double *nf;            // m-vector (nf_is_vector) or matrix
    int nf_is_vector;
    const double *dispFit;       // n
    const double *intercept;     // n (form B) or nullptr (form A)
    double lambda, lambda0;      // the ridges on the natural-log scale: samples, intercept
    double tol, minmu;
    int maxit;
    double *out;                 // n x m; beyond the LDS regime the row is the fit's scratch until the result is written
    double *intercept_out;       // n or nullptr
    double *iter;                // n
    int32_t *flag;               // n
    int32_t *bad;                // float64 counts: as VstKernelParams.bad
};
hipError_t launch_rlog(const RlogKernelParams &kp, int y_f64, hipStream_t st);

// apeglm shrinkage (apeglm.hip).  Element (i, j) of counts / nf matrix / weights sits at
// [i * si + j * sj]; map / sd / init: n x p, p contiguous per gene; iter: n x 2.
struct ApeglmKernelParams {
    int n, m, p;
    const void *y;
    long si, sj;
    const double *nf;
    int nf_is_vector;
    const double *x;             // m x p column-major
    const double *weights;       // matrix or nullptr
    const double *disp;          // n
    const double *init;          // n x p or nullptr
    int coef;
    unsigned no_shrink;
    double prior_scale, prior_df, no_shrink_scale;
    int has_threshold;
    double threshold, tol;
    int maxit;
    double *map, *sd, *fsr, *thresh, *iter, *conv, *start, *objective;
    int32_t *bad;                // float64 counts: as VstKernelParams.bad
};
constexpr int kApeXLdsDoubles = 4096;     // the design is staged in LDS while m * p doubles fit here (dsq_apeglm_lds_doubles)
hipError_t launch_apeglm(const ApeglmKernelParams &kp, int y_f64, hipStream_t st);

// adaptive shrinkage (ash.hip).  b / s and the seven per-row outputs: column c at [c * ld].
// launch_ash carves its state from the caller's workspace, runs the host loop (one record read back per evaluation and per
// line search) and returns a DSQ_* code: a column without a kept row and a grid beyond kAshMaxK are found on the way.
struct AshKernelParams {
    int n, C;
    long ld;
    const double *b, *s;
    int has_threshold;
    double threshold;
    int maxit;
    double *pm, *psd, *neg, *pos, *lfsr, *le_t, *gt_mt;
    double *pi, *sd;             // C x kAshMaxK
    int32_t *K, *iter, *flag;    // C
    double *loglik;              // C
};
constexpr int kAshMaxK = 64;            // DSQ_ASH_MAX_K
constexpr int kAshSliceRows = 128;      // dsq_ash_slice_rows(): the consecutive rows of one partial sum ...
constexpr int kAshGroupRows = 16;       // ... which adds its groups of this many rows in order
constexpr int kAshTrials = 32;          // the step sizes 0.75^j of one line search
size_t ash_workspace_bytes(long n, long C);
int launch_ash(const AshKernelParams &kp, void *workspace, hipStream_t st);

// unmix() (unmix.hip): x gene-major (element (g, i) at [g * ld + i]), pure gene-major with k
// contiguous doubles per gene; vx: the caller's workspace, m x n, written by the preparation kernel and read by the fit.
struct UnmixKernelParams {
    int n, m, k;
    long ld;
    const double *x, *pure;
    int alpha_form;              // 1: v of a negative binomial with dispersion a; 0: log(q + a)
    double a;                    // alpha or shift
    int power, maxit;
    double *vx;
    double *p;                   // m x k, k contiguous per sample
    double *loss;                // m
    int32_t *iter, *flag;        // m
};
size_t unmix_workspace_bytes(int n, int m);
hipError_t launch_unmix(const UnmixKernelParams &kp, hipStream_t st);

// the solve of estimateSizeFactors(type = "iterate") (sf_iterate.hip): y / mu gene-major, read only;
// launch_sf_iterate carves its state from the caller's workspace, runs the host loop (one small record read back per
// evaluation of F: it synchronises `st`) and writes the outputs.
struct SfIterateKernelParams {
    int n, m;
    long ld;
    const int32_t *y;
    const double *mu, *sf, *disp;
    const int32_t *rows;
    double Q;
    int maxit;
    double *s_out, *sf_out, *F_out;       // m, m, 1
    int32_t *iter_out, *evals_out, *flag_out;
};
size_t sf_iterate_workspace_bytes(long n, long m);
hipError_t launch_sf_iterate(const SfIterateKernelParams &kp, void *workspace, hipStream_t st);

// results() (results.hip): the table of one coefficient, the threshold tests, and the Benjamini-
// Hochberg adjustment over K nested filter subsets from ONE sort of the p-values.  n-vectors and n x p column-major
// matrices; the second block is carved from the caller's workspace by launch_results.
struct ResultsKernelParams {
    int n, p, c;                 // genes, design columns, the coefficient
    int lrt;                     // stat / pvalue are the n-vectors LRTStatistic / LRTPvalue (else n x p, column c)
    int alt;                     // DSQ_ALT_* of the public header; threshold: stat / pvalue are recomputed from LFC, SE, T
    int threshold;
    double T, alpha;
    const double *beta, *betaSE, *stat, *pvalue, *baseMean;
    const int32_t *replace, *na_mask;   // n flags or nullptr
    const double *filter;        // n (baseMean when the caller gave none)
    const double *theta;         // K quantile levels, or nullptr: no filtering (K = 1, every non-NA p-value adjusted)
    int K;
    double *o_baseMean, *o_lfc, *o_se, *o_stat, *o_pvalue;   // n each
    double *filtPadj;            // n x K column-major
    int32_t *numRej;             // K
    double *cutoffs;             // K
    int32_t *status;             // bit 0: NaN in filter, bit 1: a theta outside [0, 1]
    unsigned long long *keyA, *keyB;
    unsigned int *rowA, *rowB, *hist, *counters;
    const double *df;            // n degrees of freedom: the threshold tests run under Student's t (nullptr: the normal distribution)
};
hipError_t launch_results(ResultsKernelParams kp, void *workspace, hipStream_t st);
size_t results_sort_workspace_bytes(long n);     // the sort's part; filtPadj (n K doubles) may follow it
// the same pass kernels over `ncols` INDEPENDENT columns of n keys each in one launch chain (grid y = the column; the prior
// variance of beta_prior.hip sorts a batch of columns so): column c's keys at keyA + c n (keyB, rowA, rowB alike; rows may
// be nullptr), its (digit, tile) table at hist + c sort_hist_entries(n), its copy flag at const_digit + c.  Stable,
// ascending, 8 passes A -> B -> A ...: the result is back in A, B is free.
void radix_sort_columns(unsigned long long *keyA, unsigned long long *keyB, unsigned int *rowA, unsigned int *rowB,
                        unsigned int *hist, unsigned int *const_digit, int n, int ncols, hipStream_t st);
size_t sort_hist_entries(long n);                // 256 x the tiles of one column

// sample-level exploration of a resident transform (explore.hip): x gene-major, element (g, i) at
// [g * ld + i], read only.
struct RowVarsKernelParams {
    int n, m;
    long ld;
    const double *x;
    double *rowMean, *rowVar;    // n each
};
int row_vars_register_width();                   // rows of up to this many samples are read once (else swept twice)
hipError_t launch_row_vars(const RowVarsKernelParams &kp, hipStream_t st);
// the first k entries of order(rowVar, decreasing = TRUE) -- ties and NaNs by ascending row, NaNs last -- into select
size_t top_var_workspace_bytes(long n);
hipError_t launch_top_var_order(const double *rowVar, int n, int k, int32_t *select, void *workspace, hipStream_t st);
// The all-pairs sums over R rows of the m samples.  The summation order is a function of (R, m) alone: the rows are cut into
// S slices of L consecutive rows (the last one shorter), L = max(kPairMinSlice, ceil(R / max(1, kPairWork / tiles))) with
// tiles = nb (nb + 1) / 2, nb = ceil(m / kPairTile); a slice is summed in row order from +0.0, the slice partials are added in
// slice order.  So one tile of pairs is cut into up to kPairWork slices (a small m fills the device) and the partials take
// at most max(kPairWork, tiles) tiles of 32 KiB.
constexpr int kPairTile = 64, kPairMinSlice = 64, kPairWork = 2048;
enum { PAIR_DIST2 = 0, PAIR_GRAM = 1 };
struct PairSlices { int nb; long ntiles, L, S; };
void pair_slices(long R, int m, PairSlices *ps);
size_t pair_workspace_bytes(long R, int m);
struct PairKernelParams {
    int n, m;
    long ld;
    const double *x;
    int kind, root;              // PAIR_*; root: the square root of the sums (dist)
    long R;                      // rows summed
    const int32_t *rows;         // R row indices, or nullptr: rows 0 .. R - 1
    const double *centre;        // R values, entry t subtracted from row t of the list (PAIR_GRAM), or nullptr
    int nb;
    long ntiles, L, S;           // pair_slices(R, m)
    double *partial;             // pair_workspace_bytes(R, m)
    double *out;                 // m x m
};
hipError_t launch_pair_sums(const PairKernelParams &kp, hipStream_t st);

// collapseReplicates / colSums / fpm / fpkm on the resident counts (count_helpers.hip): y int32
// gene-major, element (i, j) at [i * ld + j], read only.
struct CollapseKernelParams {
    int n, m, g;
    long ld, ldo;
    const int32_t *y;
    const int32_t *members;      // m sample indices, group by group
    const int32_t *offsets;      // g + 1: group c owns members[offsets[c] .. offsets[c + 1])
    int32_t *out;                // n x g, element (i, c) at [i * ldo + c]
    int32_t *status;             // ORed: 1 a sum that is no int32, 2 a member or an offset outside the matrix
};
hipError_t launch_collapse(const CollapseKernelParams &kp, hipStream_t st);
struct ColSumsKernelParams {
    int n, m;
    long ld;
    const int32_t *y;
    long long *sums;             // m
};
hipError_t launch_col_sums(const ColSumsKernelParams &kp, hipStream_t st);
enum { FPM_FPM = 0, FPM_FPKM_BASEPAIRS = 1, FPM_FPKM_TXLEN = 2 };       // = DSQ_FPM, DSQ_FPKM_* of the public header
struct FpmKernelParams {
    int n, m;
    long ld;                     // of y, txlen and out alike
    const int32_t *y;
    int kind;
    const double *lib;           // m library sizes
    const double *basepairs;     // n (FPM_FPKM_BASEPAIRS)
    const double *txlen;         // n x m (FPM_FPKM_TXLEN)
    double *out;                 // n x m
};
hipError_t launch_fpm(const FpmKernelParams &kp, hipStream_t st);

// the local-regression dispersion trend (local_fit.hip).  The fit handle is one block of
// kLocalFitHeaderDoubles + 3 n doubles: a header (N, k, the all-below-floor flag, n, minDisp), then x | y | w of the fit set
// in sorted order, each n long (the first N entries written).  kLocalFitLanes: the partial sums of every moment -- partial
// (j mod kLocalFitLanes) takes the window's points in ascending sorted index j, then the butterfly of wave_allreduce.
constexpr int kLocalFitLanes = 64, kLocalFitHeaderDoubles = 4;
size_t local_fit_workspace_bytes(long n);        // the sort's scratch
hipError_t launch_local_fit_build(const double *means, const double *disps, int n, double minDisp, double *block, void *workspace,
                                  hipStream_t st);
// dispFit at the n_eval means q into out (out == nullptr: nothing is evaluated), then status[0..3] = N, k, singular points,
// all-below-floor
hipError_t launch_local_fit_eval(const double *block, const double *q, long n_eval, double *out, int32_t *status, hipStream_t st);

// K contrasts from one covariance pass per gene (contrasts.hip).  n x m matrices gene-major with
// leading dimension ld, n x p / n x K matrices column-major; ncell > 0 selects the cell-collapsed Gram sums (cell_perm,
// cell_start as in BetaKernelParams); contrasts == nullptr: the all-zero flags only.
struct ContrastsKernelParams {
    int n, m, p, K;
    long ld;
    const double *x, *nf;
    int nf_is_vector;
    const double *alpha_hat, *beta, *lambda, *weights;
    int useWeights;
    double minmu;
    const double *contrasts;
    const int32_t *allZero, *counts, *sample_mask, *rule_applies;
    const int32_t *cell_perm, *cell_start;
    int ncell;
    double *lfc, *se, *stat, *pvalue;
    int32_t *flags;
};
// rows of more than contrasts_max_m(p) samples do not fit the per-sample path (*ok = false, nothing launched)
hipError_t launch_contrasts(const ContrastsKernelParams &kp, hipStream_t st, bool *ok);
// pt over an n x K column-major column, df per row (student.hip); tail: DSQ_PT_* of the public header
hipError_t launch_pt(const double *q, const double *df, long n, long K, int tail, const int32_t *keep, double *out,
                     hipStream_t st);
int contrasts_max_m(int p);

// gene index of work item i, and the number of work items, of a (possibly row-listed) launch
#define DSQ_NWORK(kp) ((kp).n_dev ? *(kp).n_dev : (kp).n)
#define DSQ_GENE(kp, i) ((kp).rows ? (kp).rows[i] : (i))

hipError_t launch_cooks(const CooksKernelParams &kp, hipStream_t st, bool *ok);
hipError_t launch_replace(const ReplaceKernelParams &kp, hipStream_t st, bool *ok);
hipError_t launch_prefit(const PrefitKernelParams &kp, hipStream_t st, bool *ok);
hipError_t launch_linear_mu(const PrefitKernelParams &kp, double mu_floor, double *mu, hipStream_t st, bool *ok);
hipError_t launch_loglike(const LogLikeKernelParams &kp, hipStream_t st);
hipError_t launch_intercept_fit(const InterceptKernelParams &kp, hipStream_t st);
// trend.hip: the trend phase of the chain (DSQ_PH_TREND).  The parametric fit needs trend_fit_workspace_bytes() of device
// workspace: launch_trend_fit (n on the host) and launch_trend_fit_dev (n on the device) zero it themselves, _zeroed expects
// it zeroed; launch_prior_var needs prior_var_workspace_bytes(n) ZEROED bytes (0 below the size at which it runs on sixteen
// workgroups: no workspace then)
hipError_t launch_trend_fit(const double *means, const double *disps, long n, double *coefs, int32_t *status,
                            void *workspace, hipStream_t st);
hipError_t launch_trend_fit_dev(const double *means, const double *disps, const int32_t *n_dev, double *coefs,
                                int32_t *status, void *workspace, hipStream_t st);
hipError_t launch_trend_fit_dev_zeroed(const double *means, const double *disps, const int32_t *n_dev, double *coefs,
                                       int32_t *status, void *workspace, hipStream_t st);
size_t trend_fit_workspace_bytes();
hipError_t launch_trend_given(double *scalars, int32_t *status, hipStream_t st);
hipError_t launch_trend_mean(const double *disp, int n, double minDisp, int mode, double *scalars, int32_t *status,
                             hipStream_t st);
hipError_t launch_prior_var(const double *mean, const double *disp, int n, double minDisp, double expVarLogDisp, int m_gt_p,
                            double *resbuf, double *scalars, int32_t *status, const double *fit_in, double pv_in,
                            void *workspace, hipStream_t st);
size_t prior_var_workspace_bytes(int n);
// getAndCheckWeights on resident weights: w / rowmax, pmax(., 1e-6), the weightsFail flags, the negative-weight flag
hipError_t launch_weights_prep(const double *w_raw, const double *x, int n, int m, int p, long ld, double thr, double *w_norm,
                               double *w_floor, int32_t *force_zero, int32_t *neg, hipStream_t st);
// xim of a normalization-factor matrix -> *out (device); scratch_m: m doubles
hipError_t launch_xim(const double *nf, int n, int m, long ld, double *scratch_m, double *out, hipStream_t st);
hipError_t launch_xim_rows(const double *nf, const int32_t *rows, const int32_t *n_dev, int m, long ld, double *scratch_m,
                           double *out, hipStream_t st);

// Register-resident kernels exist for 1 <= p <= DSQ_P_REG (one translation unit per p,
// explicit specialisations in fit_disp.hip / fit_beta.hip compiled with -DDSQ_P=p).
#define DSQ_P_REG 10
// 11 <= p <= DSQ_P_WIDE run on the translation units of DSQ_WIDE_LIST (-DDSQ_P=16, 24, ...: loops not unrolled, p x p state in
// scratch memory) over designs zero-padded to the next listed width: a padded column gets ridge 1 and a unit diagonal in
// the Cox-Reid matrix, which leaves every quantity of the real coefficients unchanged (capi.hip, "wide designs").
// (round 5: 32 and 48 added -- `~ patient + treatment` with up to 47 patients, factors of up to 48 levels.  Round 6: 64 --
//  its fits are the ROLLED kernels alone (fit_beta_wide.hip, fit_disp_wide.hip: one build for every width); the per-width
//  fitDisp kernel, whose 64-column build compiles for half an hour, stops at DSQ_DISP_PERWIDTH_MAX)
#define DSQ_P_WIDE0 16
#define DSQ_WIDE_LIST(X) X(16) X(24) X(32) X(48) X(64)
#define DSQ_P_WIDE 64
#define DSQ_DISP_PERWIDTH_MAX 48
static inline unsigned long long dsq_low_bits(int k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }   // bits 0 .. k - 1
static inline int dsq_wide_width(int p) { return p <= 16 ? 16 : p <= 24 ? 24 : p <= 32 ? 32 : p <= 48 ? 48 : 64; }   // padded width of a wide p
// every design width 1 .. DSQ_P_WIDE (the small per-width kernels of aux.hip: pre-fit moments, linear mu)
#define DSQ_P_EACH(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) \
    X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35) X(36) X(37) X(38) X(39) X(40) \
    X(41) X(42) X(43) X(44) X(45) X(46) X(47) X(48) X(49) X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58) X(59) X(60) \
    X(61) X(62) X(63) X(64)
#define DSQ_CMAX 32       // most design cells the cell-collapsed paths take
#define DSQ_DISP_CELL_MINP 4   // fitDisp assembles the Cox-Reid matrices from cell sums from this design width up
template <int P> hipError_t launch_fit_disp_p(const DispKernelParams &kp, hipStream_t st, bool grid);
template <int P> hipError_t launch_fit_beta_p(const BetaKernelParams &kp, hipStream_t st);
template <int P> hipError_t launch_optim_p(const OptimKernelParams &kp, hipStream_t st);
// doubles of global scratch one fitBeta launch needs: `slab` (per-wave mu/sqrt(w)/sqrt(w)z when they
// do not fit in LDS, else 0) and `cscr` (hoisted NB-density constants)
template <int P> void fit_beta_scratch_doubles(int n, int m, int use_weights, size_t *slab, size_t *cscr);

// launch-geometry knobs (environment variables DSQ_*; read once) -- used for tuning sweeps
struct Tuning {
    int beta_waves, beta_stage, beta_bpc, beta_lds_kb;
    int disp_waves, disp_stage, disp_bpc, disp_lds_kb;
    int ablate, force_iters;
    int disp_xlds, beta_xlds;
    int dynamic;             // DSQ_DYNAMIC (default 1): dynamic gene scheduling in the fit kernels
    int beta_cells;          // DSQ_BETA_CELLS (default 1): cell-collapsed fitBeta for designs with <= DSQ_CMAX cells
    int disp_cell_minp;      // DSQ_DISP_CELL_MINP (profiling; default = the macro): fitDisp cell mode from this width up
    // the chain (pipeline.hip)
    int overlap;             // DSQ_OVERLAP (default 1): the test's full-row nbinomLogLike on a side stream beside the refit
    // launch orders of the chain's full-size fit launches (pipeline.hip: lpt_scatter_kernel; profiles/launch_order.md)
    int lpt;                 // DSQ_LPT (default 1: from 256 samples; 2: whatever the row length; 0: every launch in list order)
    int lpt_maxn;            // DSQ_LPT_MAXN (default 16384; 0: no limit): the MAP fit_disp is ordered up to n genes
    int lpt_key1;            // DSQ_LPT_KEY1 (default 1): the gene-wise fit_beta by ascending baseMean; 0: list order
    int lpt_keyd;            // DSQ_LPT_KEYD (default 1): the gene-wise fit_disp by descending baseMean (the same list backwards) for
                             // 256 <= m <= 1024 without weights; 2: always; 0: list order
    int lpt_keym;            // DSQ_LPT_KEYM (default 2): the MAP fit_disp by 2 descending baseMean, 3 the gene-wise search's iterations,
                             // 5 iterations x log2 mean, 6 |start value - prior mean|; 0: list order
    int lpt_key2;            // DSQ_LPT_KEY2 (default 1): the test's fit_beta by ascending baseMean like the gene-wise one; 0: by the
                             // gene-wise IRLS's iterations; 2: list order
    int outlier_first;       // DSQ_OUTLIER_FIRST (default 1): the rows that can hold a count outlier first, their refit beside the
                             // Cook's distances of all the others (pipeline.hip, phase_outlier_first)
    // the per-width fitDisp search (fit_disp.hip, DSQ_DISP_GAMMA)
    int disp_predict;        // DSQ_DISP_PREDICT: 1 likelihood-only evaluations where the search is predicted to reject; 0 fused at
                             // every proposal; 2 likelihood-only at every proposal, fused after each acceptance that continues.
                             // Same bits under all three.  Unset (-1): 1, but 0 for the shape gated in launch_disp_p
                             // (fit_disp.hip): unweighted rows of a two-column design with up to 100 samples, measured at C2
                             // (100 samples; shorter rows are an extrapolation, said there).  Rule for a gate: a shape keeps
                             // policy 0 only where a paired measurement shows policy 1 losing there
                             // (profiles/disp_predict.md); the knob, when set, holds for every shape
};
const Tuning &tuning();

hipError_t launch_transpose_r_to_gm_f64(const double *src, double *dst, int n, int m, long ld, hipStream_t st);
hipError_t launch_transpose_r_to_gm_i32(const int32_t *src, int32_t *dst, int n, int m, long ld, hipStream_t st);
hipError_t launch_counts_f64_to_gm_i32(const double *src, int32_t *dst, int n, int m, long ld, int32_t *bad, hipStream_t st);
hipError_t launch_transpose_gm_to_r_f64(const double *src, double *dst, int n, int m, long ld, hipStream_t st);
hipError_t launch_transpose_gm_to_r_i32(const int32_t *src, int32_t *dst, int n, int m, long ld, hipStream_t st);
hipError_t launch_test_math(int op, const double *a, const double *b, const double *c, double *out, long n, hipStream_t st);

constexpr int kMaxDevices = 64;      // device indices the per-device tables take (device_cu_count, stage.hip)
int device_cu_count();
// launch-geometry caches are per host thread (the multi-device host entry points drive one device per worker thread)
// and are dropped when that thread moves to another device: the MaxDynamicSharedMemorySize attribute and the occupancy
// figure belong to a device
#define DSQ_CACHE_PER_DEVICE(a, b)                                                        \
    do {                                                                                  \
        static thread_local int cache_dev_ = -1;                                          \
        int dev_now_ = 0;                                                                 \
        (void)hipGetDevice(&dev_now_);                                                    \
        if (dev_now_ != cache_dev_) { memset(a, 0, sizeof a); memset(b, 0, sizeof b); cache_dev_ = dev_now_; } \
    } while (0)

// ---- host side: shared by the C ABI files (ctx.hip, capi.hip, capi_host.hip) and the chain (pipeline.hip, deseq_host.hip) ----
int capi_fail(int code, const char *fmt, ...);                   // sets this thread's dsq_last_error() text, returns code
extern thread_local char g_err[512];                             // that text
#define DSQ_HIP(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return capi_fail(e_ == hipErrorOutOfMemory ? DSQ_ERR_NOMEM : DSQ_ERR_DEVICE, "%s: %s", #expr, \
                             hipGetErrorString(e_));                                             \
    } while (0)
int env_int(const char *name, int dflt);
// ctx.hip: everything that belongs to "the stream this call runs on" -- the workspace slots (table cache included), the
// pinned upload ring with its events, the side stream -- sits in one StreamCtx per (device, stream).  An entry point
// (WsScope / capi_latch_stream, under the call lock) and a worker thread of a host call (at the start of every job)
// resolve the context ONCE and latch a pointer to it for their thread; the functions below work on the latched
// context without a lock: a context is only ever used by the thread that latched it.  dsq_release_workspace() destroys
// the contexts, so a latch is never kept across calls.
extern std::mutex g_mu;                                          // the library's call lock
void capi_latch_stream(hipStream_t s);
int capi_ws_get(int slot, size_t bytes, void **out);             // grow-only workspace slot of the latched context
int capi_upload_table(int slot, const void *src, size_t bytes, hipStream_t st, void **dev_out);   // small host table -> slot (pinned ring, skipped when unchanged)
int capi_check_device();
int capi_upload_cells(const int32_t *labels, int m, int slot, hipStream_t st, const int32_t **perm_dev,
                      const int32_t **start_dev);
// the rolled kernel of the wide designs without design cells (fit_beta_wide.hip): any kp.p in 11 .. 64
hipError_t launch_fit_beta_rolled(const BetaKernelParams &kp, hipStream_t st);
void fit_beta_rolled_scratch_doubles(int n, int m, int p, int useW, size_t *slab, size_t *cscr);
hipError_t dispatch_fit_beta(int p, const BetaKernelParams &kp, hipStream_t st, bool *ok);
// a fit at the (kernel) width p with ncell design cells runs on the cell kernel -- the one that writes BetaKernelParams.cand_flag
static inline bool fit_beta_on_cells(int p, int ncell) { return p <= 32 /* DSQ_SPEC_BETA_CELL_MAXP */ && ncell > 0 && ncell <= DSQ_CMAX && ncell + p <= 64; }
void dispatch_beta_scratch(int p, int n, int m, int useW, size_t *slab, size_t *cscr);
hipError_t dispatch_fit_disp(int p, const DispKernelParams &kp, hipStream_t st, bool grid, bool *ok);
bool fit_disp_rolled_applies(const DispKernelParams &kp, int *p_true);       // fit_disp_wide.hip
hipError_t dispatch_optim_rows(int p, const OptimKernelParams &kp, hipStream_t st, bool *ok);
void capi_prof_begin(const char *name, int n, hipStream_t st);   // no-ops unless dsq_profile_enable(1)
void capi_prof_end(hipStream_t st);
bool capi_prof_on();
// a second stream (with two events) next to the latched context's: the chain runs work that nothing downstream waits for
// beside its serial tail (pipeline.hip); created on first use
int capi_side_stream(hipStream_t *side, hipEvent_t *fork_ev, hipEvent_t *join_ev);
// the gene ranges of a host-pointer call (capi_host.hip); the caller holds the call lock
int capi_host_sharded(size_t n, const std::function<int(size_t, size_t, hipStream_t, int, int)> &f, int max_shards);
int capi_host_shards(size_t n);
// stage.hip: pageable host memory <-> device through pinned chunks packed by a small thread pool; rows [lo, lo + cnt) of
// a column-major n_total x cols host matrix <-> a contiguous column-major cnt x cols device matrix.  stage_d2h returns
// when the host rows are complete.
int stage_h2d(void *dev, const void *host, size_t e, size_t n_total, size_t lo, size_t cnt, size_t cols, hipStream_t st);
int stage_d2h(void *host, const void *dev, size_t e, size_t n_total, size_t lo, size_t cnt, size_t cols, hipStream_t st);
// first touch of a large result matrix in the caller's (fresh, pageable) memory on helper threads, ahead of the copy into
// it -- announce the outputs when an entry point starts, wait before it returns (stage.hip)
void stage_prefault(void *host, size_t bytes);
void stage_prefault_finish();
struct PrefaultScope { ~PrefaultScope() { stage_prefault_finish(); } };
// an entry point's scope: latches the context of its stream (under g_mu); on the way out it waits for the first-touch
// threads of stage.hip -- no entry point returns while they are at work
struct WsScope { explicit WsScope(hipStream_t s) { capi_latch_stream(s); } ~WsScope() { stage_prefault_finish(); } };
// (three slots between the call slots of capi.hip and the chain's: the padded reduced / prior design, the padded design, the
//  prior-variance selection workspace)
enum { DSQ_WS_PIPE_PADXR = 37, DSQ_WS_PIPE_PADX = 38, DSQ_WS_PIPE_SEL = 39 };
// (DSQ_WS_PIPE_META: the trend fit's workspace; behind it the outlier tables, the design cells of the full and the reduced
//  model, the reduced / prior fit's fitted means, the column sums behind xim)
enum { DSQ_WS_PIPE = 40, DSQ_WS_PIPE_SCRATCH = 41, DSQ_WS_PIPE_META = 42, DSQ_WS_PIPE_OUTLIER_META = 43, DSQ_WS_PIPE_CELLS = 44,
       DSQ_WS_PIPE_CELLS_RED = 45, DSQ_WS_PIPE_RED_MU = 46, DSQ_WS_PIPE_XIM_SCRATCH = 47, DSQ_WS_HOSTDESEQ = 48, DSQ_WS_COUNT = 72 };

}  // namespace dsq
