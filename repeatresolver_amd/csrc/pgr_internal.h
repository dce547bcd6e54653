/* pgr_internal.h -- what pgr_host.c and the pgr_*_device.hip files share inside libpwr.so; not part of the C ABI. */
#ifndef PGR_INTERNAL_H
#define PGR_INTERNAL_H

#include "pgr.h"

/* The MSA resident on the device (pgr_msa_open, pgr_win_device.hip); pgr_cons_device.hip reads the text too */
struct pgr_msa {
    int rows, width, device;
    unsigned char *text;              /* [rows][width] on the device */
};

/* A window's sets on the device, word-major as k_gr_cliques and k_gr_votes read them */
typedef struct {
    int rows, kept_rows, von, bis, width, sc;
    const unsigned long long *G;      /* [sc][width * 5] */
    const unsigned long long *LC;     /* [sc][width] */
    const int *gsize;                 /* [width * 5] rows of every group */
} pgr_device_sets;

/* pgr_refine from the MaxCorrs slice on, on sets that are on the device already; kept[rows] and coverage[width] on the
 * host.  msa_width = the width of the whole MSA (maxcorrs_full[msa_width * 5]).  *result as pgr_refine leaves it (freed on
 * failure); ms2 (may be NULL): [0] cliques, [1] votes. */
__attribute__((visibility("hidden"))) int pgr_refine_sets(const pgr_device_sets *sets, const unsigned char *kept, const int *coverage,
                                                          const double *maxcorrs_full, int msa_width, int mincov, double cutoff, int device,
                                                          pgr_result *result, double *ms2);

/* Set-major to word-major, as the kernels read a window's sets: out[w * n + c] = sets[pick[c] * sc + w] for the n sets
 * pick[0 .. n) of sc words each (pick = NULL: all of them, pick[c] = c).  out[sc * n].  It is a transposition, so the way
 * back is the same call with the two extents exchanged: pgr_word_major(word_major, n, NULL, sc, set_major). */
#ifdef __cplusplus
extern "C"
#endif
__attribute__((visibility("hidden"))) void pgr_word_major(const unsigned long long *sets, int sc, const int *pick, size_t n,
                                                          unsigned long long *out);
#endif
