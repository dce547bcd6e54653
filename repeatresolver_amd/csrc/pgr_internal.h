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

#ifdef __cplusplus
#include <vector>

/* What pgr_msa_consensus and pgr_msa_settle do with a labelling and a window before anything else: von == bis == -1 is the
 * whole width.  The largest label, or PWR_ERR_ARG for a window outside the text, a label below -1 or no label at all, or
 * PWR_ERR_RANGE for a label from PGR_MAX_ROWS on. */
static inline int pgr_window_and_top(const int *labels, int rows, int width, int *von, int *bis)
{
    if (*von == -1 && *bis == -1) { *von = 0; *bis = width - 1; }
    if (*von < 0 || *bis >= width || *von > *bis) return PWR_ERR_ARG;
    int top = -1;
    for (int r = 0; r < rows; ++r) {
        if (labels[r] < -1) return PWR_ERR_ARG;
        if (labels[r] > top) top = labels[r];
    }
    if (top >= PGR_MAX_ROWS) return PWR_ERR_RANGE;
    return top < 0 ? PWR_ERR_ARG : top;
}

/* SignaturesMaker's columns of [von, bis] (TA:263, TA:157), in doubles on the host: those whose largest of the five MaxCorrs
 * exceeds the cutoff; every column where maxcorrs_full is null */
static inline std::vector<int> pgr_signature_columns(int von, int bis, const double *maxcorrs_full, double cutoff)
{
    std::vector<int> columns;
    for (int x = von; x <= bis; ++x) {
        bool in = true;
        if (maxcorrs_full) {
            double m = maxcorrs_full[(size_t)x * 5];
            for (int i = 1; i < 5; ++i) if (maxcorrs_full[(size_t)x * 5 + i] > m) m = maxcorrs_full[(size_t)x * 5 + i];
            in = m > cutoff;
        }
        if (in) columns.push_back(x);
    }
    return columns;
}
#endif
#endif
