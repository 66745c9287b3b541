// student.hip -- Student's t distribution function over an n x K column.
//
// One thread per entry: out[i + n k] = pt(q[i + n k], df[i]) in the tail asked for (dsq_math.hpp: dpt_upper / dpt_lower),
// row i's degrees of freedom for every column.  Entries whose `keep` flag is set are left as they are -- the rows the
// all-zero rule of cleanContrast has already set to 1 (R/results.R:1024-1028 runs after getContrast's p-value).  An entry
// reads only itself, so out may be q.  dsq_contrasts_dev runs this pass behind its kernel on a useT analysis: the p-value
// there sits on one lane in p, and an iterative function on that lane would idle the rest of the wave.
#include "../../include/deseq2_mi355x.h"
#include "dsq_internal.hpp"
#include "dsq_math.hpp"

namespace dsq {

__global__ void __launch_bounds__(256) pt_kernel(const double *q, const double *df, long n, long total, int tail,
                                                 const int32_t *keep, double *out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    if (keep && keep[e] != 0) return;
    const double v = q[e], d = df[e % n];
    double r;
    if (tail == DSQ_PT_LOWER) r = dpt_lower(v, d);
    else if (tail == DSQ_PT_UPPER) r = dpt_upper(v, d);
    else r = 2.0 * dpt_upper(__builtin_fabs(v), d);          // 2 * pt(abs(q), df, lower.tail = FALSE), R/results.R:814
    out[e] = r;
}

hipError_t launch_pt(const double *q, const double *df, long n, long K, int tail, const int32_t *keep, double *out,
                     hipStream_t st) {
    const long total = n * K;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q, df, n, total, tail, keep, out);
    return hipGetLastError();
}

}  // namespace dsq
