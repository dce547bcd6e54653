/* TEST INFRASTRUCTURE -- NOT PRODUCT CODE.
 *
 * The three functions of oracle/gsl_standin/gsl/gsl_cdf.h (see there for the reference's call sites).  The two
 * hypergeometric tails are mco_hyper_Q / mco_hyper_P of oracle/mc_oracle.c -- the tail that tests/test_mc_oracle.py pins
 * against scipy and exact rationals; there is no second copy here, this file is linked together with mc_oracle.c.  The
 * binomial tail is a plain sum of its terms.  tests/test_rr_reference.py compares all three with scipy.
 */
#include <math.h>

#include "gsl/gsl_cdf.h"

double mco_hyper_Q(unsigned k, unsigned n1, unsigned n2, unsigned t);
double mco_hyper_P(unsigned k, unsigned n1, unsigned n2, unsigned t);

double gsl_cdf_hypergeometric_Q(const unsigned int k, const unsigned int n1, const unsigned int n2, const unsigned int t)
{
    return mco_hyper_Q(k, n1, n2, t);
}

double gsl_cdf_hypergeometric_P(const unsigned int k, const unsigned int n1, const unsigned int n2, const unsigned int t)
{
    return mco_hyper_P(k, n1, n2, t);
}

/* P(X > k) = sum over i in (k, n] of C(n, i) p^i (1 - p)^(n - i): all terms are positive, so the sum keeps the relative
 * precision of its terms however small the tail is */
double gsl_cdf_binomial_Q(const unsigned int k, const double p, const unsigned int n)
{
    if (k >= n) return 0.0;
    if (p <= 0.0) return 0.0;
    if (p >= 1.0) return 1.0;
    const double lp = log(p), lq = log1p(-p), ln1 = lgamma(n + 1.0);
    double Q = 0.0;
    for (unsigned i = k + 1; i <= n; i++)
        Q += exp(ln1 - lgamma(i + 1.0) - lgamma(n - i + 1.0) + i * lp + (n - i) * lq);
    return Q;
}
