// hyper_tail.h -- the upper tail of the hypergeometric distribution on the device, shared by pmc_device.hip (MaxCorrelation)
// and pgr_device.hip (RepeatResolver's group refinement).  It follows GSL's scheme (sum of pdf terms by ratio recurrences
// away from k; pdf = exp of three lnchoose): equal to gsl_cdf_hypergeometric_Q up to rounding of lgamma / exp, not bit for bit.
#ifndef PWR_HYPER_TAIL_H
#define PWR_HYPER_TAIL_H

#include <hip/hip_runtime.h>

// lnf[n] = lgamma(n + 1), n <= rows (made on the host: no count exceeds the number of rows)
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

// gsl_cdf_hypergeometric_Q(k, n1, n2, t) = P(X > k)
static __device__ double d_hyper_Q(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t)
{
    if (k >= n1 || k >= t) return 0.0;
    const double midpoint = ((double)t * n1) / ((double)n1 + n2);
    if (k < midpoint) {
        unsigned i = k;
        double s = d_hyper_pdf(lnf, i, n1, n2, t), P = s;
        while (i > 0) {
            s *= (i / (n1 - i + 1.0)) * ((n2 + i - t) / (t - i + 1.0));
            P += s;
            if (s / P < 2.2204460492503131e-16) break;
            i--;
        }
        return 1.0 - P;
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

// gsl_cdf_hypergeometric_P(k, n1, n2, t) = P(X <= k): the same two sums, the other way round (used by the k-means stage's
// relative significance only, RR:492)
[[maybe_unused]] static __device__ double d_hyper_P(const double *__restrict__ lnf, unsigned k, unsigned n1, unsigned n2, unsigned t)
{
    if (k >= n1 || k >= t) return 1.0;
    const double midpoint = ((double)t * n1) / ((double)n1 + n2);
    if (k < midpoint) {
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
    return 1.0 - Q;
}

#endif /* PWR_HYPER_TAIL_H */
