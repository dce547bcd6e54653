/* TEST INFRASTRUCTURE -- NOT PRODUCT CODE.
 *
 * Stand-in for <gsl/gsl_cdf.h>: the three GSL functions the reference's MaxCorrelation.c ("MC:") and RepeatResolver.c
 * ("RR:") call, so that `make -C oracle ref` can compile both UNMODIFIED (-I oracle/gsl_standin) where GSL is not
 * installed.  Defined in oracle/gsl_standin.c; nothing under repeatresolver_amd/ includes or links this.
 *
 * Call sites in the reference, and whether their value reaches an output file:
 *   gsl_cdf_hypergeometric_Q  MC:415  PositiveCumHypGeo_Log -> PositiveSignificance -> every line of MaxCorrsOf_*: REACHES.
 *                             RR:451  PositiveCumHypGeo_Log -> Group_PositiveSignificance -> Cliquer's ranking -> the cliques
 *                                     -> both DropoffSubdivisionOf_* and RelDropSubdivisionOf_*: REACHES.
 *                             MC:458, RR:493  CumHypGeo_Log, see below.
 *   gsl_cdf_hypergeometric_P  MC:457  CumHypGeo_Log -> Relative_Group_Significance, which MaxCorrelation never calls: does not.
 *                             RR:492  CumHypGeo_Log -> Relative_Group_Significance -> Relative_Vars -> Kmeans_Subdivision, which
 *                                     runs after the two drop-off files are written (RR:4065): reaches only
 *                                     KmeansSubdivisionOf_*, which is not ported and not recorded.
 *   gsl_cdf_binomial_Q        MC:491  Erwartete_Anzahl_... -> BestCutoff, which MaxCorrelation never calls: does not.
 *                             RR:526  Erwartete_Anzahl_... -> BestCutoff (RR:1659): called for every refined variation, but
 *                                     its result is overwritten by Dropoff_Cutoff two lines on (RR:1661): does not.
 */
#ifndef ORACLE_GSL_STANDIN_CDF_H
#define ORACLE_GSL_STANDIN_CDF_H

#ifdef __cplusplus
extern "C" {
#endif

/* P(X > k), X = successes among t draws without replacement from n1 successes and n2 failures */
double gsl_cdf_hypergeometric_Q(const unsigned int k, const unsigned int n1, const unsigned int n2, const unsigned int t);
/* P(X <= k) */
double gsl_cdf_hypergeometric_P(const unsigned int k, const unsigned int n1, const unsigned int n2, const unsigned int t);
/* P(X > k), X = successes among n trials of probability p */
double gsl_cdf_binomial_Q(const unsigned int k, const double p, const unsigned int n);

#ifdef __cplusplus
}
#endif
#endif
