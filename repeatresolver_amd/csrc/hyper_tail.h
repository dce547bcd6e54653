// hyper_tail.h -- the upper tail of the hypergeometric distribution on the device, shared by pmc_device.hip (MaxCorrelation),
// pgr_device.hip (RepeatResolver's group refinement) and pgr_km_device.hip (its k-means stage).  It follows GSL's scheme
// (sum of pdf terms by ratio recurrences away from k; pdf = exp of three lnchoose): equal to gsl_cdf_hypergeometric_Q up to
// rounding of lgamma / exp, not bit for bit.
#ifndef PWR_HYPER_TAIL_H
#define PWR_HYPER_TAIL_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

// lnf[n] = lgamma(n + 1), n <= rows + 1 (hyper_lnf_table below)
__device__ __forceinline__ double d_lnchoose(const double *__restrict__ lnf, unsigned n, unsigned m)
{
    if (m == n || m == 0) return 0.0;
    return lnf[n] - lnf[m] - lnf[n - m];
}

__device__ __forceinline__ double d_ln_hyper_pdf(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t)
{
    return d_lnchoose(lnf, n1, k) + d_lnchoose(lnf, n2, t - k) - d_lnchoose(lnf, n1 + n2, t);
}

__device__ __forceinline__ double d_hyper_pdf(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t)
{
    if (t > n1 + n2) t = n1 + n2;
    if (k > n1 || k > t) return 0.0;
    if (t > n2 && k + n2 < t) return 0.0;
    return exp(d_ln_hyper_pdf(lnf, k, n1, n2, t));
}

// The sum both tails are made of, terms by ratio recurrences away from k: below the midpoint from k downward (*lower = true:
// the sum is P(X <= k)), else from k + 1 upward (the sum is P(X > k)).
__device__ __forceinline__ double d_hyper_sum(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t, bool *lower)
{
    const double midpoint = ((double)t * n1) / ((double)n1 + n2);
    *lower = k < midpoint;
    if (*lower) {
        unsigned i = k;
        double s = d_hyper_pdf(lnf, i, n1, n2, t), P = s;
        while (i > 0) {
            s *= (i / (n1 - i + 1.0)) * ((n2 + i - t) / (t - i + 1.0));
            P += s;
            if (s / P < 2.2204460492503131e-16) break;
            i--;
        }
        return P;
    }
    unsigned i = k + 1;
    double s = d_hyper_pdf(lnf, i, n1, n2, t), Q = s;
    while (i < t) {
        s *= ((n1 - i) / (i + 1.0)) * ((t - i) / (n2 + i + 1.0 - t));
        Q += s;
        if (s / Q < 2.2204460492503131e-16) break;
        i++;
    }
    return Q;
}

// gsl_cdf_hypergeometric_Q(k, n1, n2, t) = P(X > k)
[[maybe_unused]] static __device__ double d_hyper_Q(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t)
{
    if (k >= n1 || k >= t) return 0.0;
    bool lower;
    const double sum = d_hyper_sum(lnf, k, n1, n2, t, &lower);
    return lower ? 1.0 - sum : sum;
}

// gsl_cdf_hypergeometric_P(k, n1, n2, t) = P(X <= k) (used by the k-means stage's relative significance only, RR:492)
[[maybe_unused]] static __device__ double d_hyper_P(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t)
{
    if (k >= n1 || k >= t) return 1.0;
    bool lower;
    const double sum = d_hyper_sum(lnf, k, n1, n2, t, &lower);
    return lower ? sum : 1.0 - sum;
}

// -log10 of the upper tail of the intersection size `schnitt` of a group of gr1 and a group of gr2 among cov rows, capped at
// 99: what PositiveSignificance (MC:413-434) and Group_PositiveSignificance (RR:472-488) share in front of their own
// saturated value.  `floor`: what the value has to reach to matter to the caller.  The tail is at least its first term, so
// -log10 pdf(schnitt) bounds the result from above: a pair below the floor is dropped before the sum (0).  Beyond 97.9 the
// callers replace the value, which the first term does not bound.  Not inlined: the kernels call it from unrolled loops over
// register arrays.
[[maybe_unused]] static __device__ __noinline__ double d_tail_z(const double *__restrict__ lnf, int schnitt, int cov, int gr1, int gr2, double floor)
{
    if (gr1 == 0 || gr2 == 0 || schnitt < 1) return 0.0;
    if (schnitt <= gr2 && schnitt <= gr1 && gr1 - schnitt <= cov - gr2) {
        const double zb = d_ln_hyper_pdf(lnf, (unsigned)schnitt, (unsigned)gr2, (unsigned)(cov - gr2), (unsigned)gr1) * -0.43429448190325182;
        if (zb < floor - 1e-6 && zb < 97.9) return 0.0;
    }
    double Z = -1.0 * log10(d_hyper_Q(lnf, (unsigned)(schnitt - 1), (unsigned)gr2, (unsigned)(cov - gr2), (unsigned)gr1));
    if (isinf(Z) || Z > 99) Z = 99.0;
    return Z;
}

// the table the functions above read, made on the host for a window of `rows` rows: no count exceeds the number of rows
[[maybe_unused]] static std::vector<double> hyper_lnf_table(int rows)
{
    std::vector<double> lnf((size_t)rows + 2);
    for (int n = 0; n < rows + 2; ++n) lnf[n] = std::lgamma(n + 1.0);
    return lnf;
}

// What the three stages' callers can hand to the functions above, for the test hooks (p*_tail_probe) that evaluate them on
// chosen counts: n tuples (schnitt, cov, gr1, gr2, size1, size2).  The lnf lookups have no bounds check of their own; inside
// these inequalities every index is a count between 0 and cov.  *maxcov: the largest cov, what the table has to reach.
[[maybe_unused]] static bool hyper_probe_counts_ok(int n, const int *counts, int max_rows, int *maxcov)
{
    if (n <= 0 || n > (1 << 24) || !counts) return false;
    int mc = 0;
    for (int t = 0; t < n; ++t) {
        const int *c = counts + (size_t)t * 6;
        const int s = c[0], cov = c[1], g1 = c[2], g2 = c[3], z1 = c[4], z2 = c[5];
        if (s < 0 || g1 < 0 || g2 < 0 || s > g1 || s > g2) return false;               // 0 <= schnitt <= min(gr1, gr2)
        if (cov > max_rows || g1 > cov || g2 > cov) return false;                      // max(gr1, gr2) <= cov <= rows
        if ((long long)s < (long long)g1 + g2 - cov) return false;                     // the two groups fit into cov rows
        if (z1 < g1 || z2 < g2 || z1 > max_rows || z2 > max_rows) return false;        // gr <= size <= rows
        if (cov > mc) mc = cov;
    }
    *maxcov = mc;
    return true;
}

// The host side of a test hook: refuses before any launch what hyper_probe_counts_ok refuses, builds the table as the stages
// do, and hands the device copies to `launch(n, counts, floor or null, lnf, out)`, the including file's own probe kernel
// (one thread per tuple, nout doubles each) -- compiled with that file's flags, which is the point.  Needs dev_util.h.
template <class Launch>
static int hyper_probe_run(int n, const int *counts, const double *floor, int device, int max_rows, int nout, double *out, Launch launch)
{
    int maxcov = 0;
    if (!out || !hyper_probe_counts_ok(n, counts, max_rows, &maxcov)) return PWR_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
    const std::vector<double> lnf = hyper_lnf_table(maxcov);
    DevArena dev;
    const int *d_counts = dev.put(counts, (size_t)n * 6);
    const double *d_floor = floor ? dev.put(floor, (size_t)n) : nullptr;
    const double *d_lnf = dev.put(lnf.data(), lnf.size());
    double *d_out = dev.get<double>((size_t)n * nout);
    if (!d_counts || (floor && !d_floor) || !d_lnf || !d_out) return dev.err;
    launch(n, d_counts, d_floor, d_lnf, d_out);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out, d_out, (size_t)n * nout * sizeof(double), hipMemcpyDeviceToHost));
    return PWR_OK;
}

#endif /* PWR_HYPER_TAIL_H */
