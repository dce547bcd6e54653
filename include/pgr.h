/*
 * pgr.h -- C ABI of the MI355X-native group refinement of RepeatResolver (part of libpwr.so), the first stage of the tool
 * that consumes MaxCorrelation's output.
 *
 * Reference: PhilippBongartz/RepeatResolver, RepeatResolver.c ("RR:").  Of its main() (RR:3863-4095) this is everything up
 * to and including Group_Refinement (RR:1634-1690; Parallel_Group_Refinement, RR:1695-1821, is the same loop dealt to
 * threads): the window reader (Einlesen, RR:293-429), the MaxCorrs slice (RR:609-646), the default cutoff and the coverage
 * restriction (RR:3977-4014), and for every significant variation its clique (Cliquer, RR:1179-1240), Sizes, the cutoff
 * of the smallest drop (Dropoff_Cutoff, RR:1460-1522) and the refined group and coverage (CliqueGroup, RR:976-1008,
 * CliqueCoverage, RR:1064-1096).  The subdivision stages that follow in the reference work on these arrays and are not
 * part of this library.  BestCutoff and KorrMaxCutoff (RR:1659-1660) are left out: their results are overwritten by
 * RR:1661 and they have no other effect.
 *
 * Floating point: only the ranking of the clique's candidates touches it (the hypergeometric tail, as in pmc.h: equal to
 * the reference's up to rounding, not bit for bit); everything else is integer arithmetic or one division of integers.
 * Error codes are those of pwr.h.
 */
#ifndef PGR_H
#define PGR_H

#include "pwr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGR_MAX_COLUMNS 1500000  /* RR:18 Max_Var_Anzahl */
#define PGR_MAX_ROWS 30000       /* RR:19 Max_Sig_Anzahl */
#define PGR_MAXCLIQUE 30         /* RR:4021: the variation itself and its 29 best partners; Clique[30] = -1 (RR:1229) */

/* The window of the MSA as Einlesen leaves it.  Bit r of a set is the r-th KEPT row (RR:332, RR:410). */
typedef struct {
    int rows, kept_rows;              /* realsigno, signumber */
    int von, bis, width;              /* bis after clipping to the line (RR:328); width = bis + 1 - von (RR:374) */
    int sc;                           /* kept_rows / 64 + 1 words per set (RR:375) */
    unsigned char *kept;              /* [rows] 1 = kept, 0 = left out (Ausgelassen 1 / -1, RR:333, RR:365) */
    unsigned long long *groups;       /* [width * 5][sc] Groups (RR:410) */
    unsigned long long *local_coverage; /* [width][sc] LocalCoverage (RR:416) */
    int *coverage;                    /* [width] Coverage (RR:417) */
} pgr_window;

/* What Group_Refinement fills, for the nsig variations whose MaxCorrs exceed the cutoff, ascending. */
typedef struct {
    int rows, kept_rows, width, sc, nsig;
    double cutoff;                    /* the one used (RR:3977) */
    unsigned char *kept;              /* [rows] */
    double *maxcorrs;                 /* [width * 5] after RR:4011-4014 and the zeroing of RR:1686 */
    int *significant;                 /* [nsig] the variation index of each entry */
    int *sizes;                       /* [nsig] Sizes (RR:1650) */
    int *cliques;                     /* [nsig][PGR_MAXCLIQUE + 1], -1 padded */
    int *cutoffs;                     /* [nsig] Cutoffs (0 where Sizes <= 5) */
    double *drop_off;                 /* [nsig] Drop_Off (1000.0 where Sizes <= 5, RR:1645) */
    unsigned long long *c_groups;     /* [nsig][sc] C_Groups (all zero where Sizes <= 5: NULL in the reference) */
    unsigned long long *c_coverage;   /* [nsig][sc] C_Coverage */
} pgr_result;

/* main() up to Group_Refinement on text = rows x width characters and the MaxCorrs vector of the WHOLE MSA
 * (maxcorrs_full[width * 5]); von = bis = -1: the whole width (RR:3948-3952).  mincov = the reference's -c, cutoff its -t
 * (below 0.1: the default of RR:3977; above 100: PWR_ERR_ARG, the trim of RR:1231 relies on Best_Corrs[0] = 100).
 * *result is filled with malloc'ed arrays: release them with pgr_free. */
int pgr_refine(int rows, int width, const unsigned char *text, const double *maxcorrs_full, int von, int bis, int mincov,
               double cutoff, int device, pgr_result *result);
void pgr_free(pgr_result *result);
/* Duration of the last pgr_refine, ms: [0] all, [1] bit sets (host reader + upload), [2] cliques, [3] votes; [4] pairs (a, i)
 * evaluated.  (Kept per process, not per call.) */
int pgr_last_timing(double *ms5);

/* ---- host side, plain C (pgr_host.c) ---- */
/* Einlesen (RR:293-429) */
int pgr_read_window(int rows, int width, const unsigned char *text, int von, int bis, pgr_window *win);
void pgr_window_free(pgr_window *win);
/* MaxCorrsEinlesen's selection (RR:631): the entries i with von <= i / 5 <= bis of full[nfull] into out[(bis + 1 - von) * 5] */
int pgr_slice_maxcorrs(const double *full, int nfull, int von, int bis, double *out);
/* MaxCorrsEinlesen (RR:609-646) from the MaxCorrsOf_ text file; *out is malloc'ed, *n = entries read */
int pgr_read_maxcorrs_file(const char *path, int von, int bis, double **out, int *n);
/* RR:3977 */
double pgr_default_cutoff(double cutoff, int width);
/* RR:4003-4014: zeroes maxcorrs[i] where coverage[i / 5] * 10 < maxcov * 9; *maxcov = the maximum of coverage */
int pgr_restrict_coverage(int width, const int *coverage, double *maxcorrs, int *maxcov);

#ifdef __cplusplus
}
#endif
#endif /* PGR_H */
