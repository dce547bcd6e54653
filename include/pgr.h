/*
 * pgr.h -- C ABI of the MI355X-native group refinement of RepeatResolver (part of libpwr.so), the first stage of the tool
 * that consumes MaxCorrelation's output.
 *
 * Reference: PhilippBongartz/RepeatResolver, RepeatResolver.c ("RR:").  Of its main() (RR:3863-4095) this is everything up
 * to and including Group_Refinement (RR:1634-1690; Parallel_Group_Refinement, RR:1695-1821, is the same loop dealt to
 * threads): the window reader (Einlesen, RR:293-429), the MaxCorrs slice (RR:609-646), the default cutoff and the coverage
 * restriction (RR:3977-4014), and for every significant variation its clique (Cliquer, RR:1179-1240), Sizes, the cutoff
 * of the smallest drop (Dropoff_Cutoff, RR:1460-1522) and the refined group and coverage (CliqueGroup, RR:976-1008,
 * CliqueCoverage, RR:1064-1096).  BestCutoff and KorrMaxCutoff (RR:1659-1660) are left out: their results are overwritten
 * by RR:1661 and they have no other effect.
 *
 * On these arrays work the first two subdivision stages (main(), RR:4026-4062), which partition the kept rows into repeat
 * copies: DropOff_Subdivision (RR:3180-3271) and RelativeDropoff_Subdivision (RR:3274-3378) with their helpers
 * (Unterteilungskomprimierung RR:1823-1843, UnterteilungsKomplettierung RR:1845-1865, Relative_Dropoff_Cutoff RR:2859-2920,
 * Unterteilung_Rausschreiben RR:568-585): the lower half of this header.  Unterteilung_Assessment (RR:2824-2856) only
 * prints and is left out.  The last stage, Kmeans_Subdivision (RR:3382-3403) with Relative_Vars (RR:2424-2493),
 * Relative_Group_Significance / CumHypGeo_Log (RR:490-522) and Kmeans (RR:2604-2821), closes the header; the drop-in
 * `RepeatResolver` binary (repeat_resolver_main.c) chains all of it and writes the reference's three label files.
 *
 * At the end: the whole repeat.  pgr_msa_* keep the MSA on the device, read every window there (pgr_win_device.hip) and run
 * the three stages per window in one call; pgr_connect chains the windows' labellings into the connection matrix of the
 * reference's SimDataAssessment.py (ProbabilityMatrix, MultiStepResolution: "SDA:" 359-391).  Last, for a labelling of the
 * rows, the consensus of every part and the differences between them on the device copy (pgr_cons_device.hip), and on those
 * the resolvability count of the reference's TransposonAssessment.py ("TA:"); and the way back, every row against every
 * part's consensus (pgr_assign_device.hip), which the reference does not have; nor has it the iteration of the two
 * (pgr_settle_device.hip), the same comparison segment by segment with every row's best crossover between two parts
 * (pgr_cross_device.hip) and the windows' labellings threaded into whole copies (pgr_thread, host).
 *
 * Floating point: only the ranking of the clique's candidates touches it (the hypergeometric tail, as in pmc.h: equal to
 * the reference's up to rounding, not bit for bit) and, in the k-means stage, the choice of the variables (both tails, against
 * the cutoff); everything else is integer arithmetic or one division of integers.
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

/* ---- the drop-off subdivisions (RR:4026-4062) ---- */
/* Both stages select the entries s with maxcorrs[significant[s]] > cutoff (RR:3188, RR:3281; sizecutoff = -1), constants as
 * in main(): mingroup = mincov / 2, dropoffcutoff = 0.0001. */
typedef struct {
    int rows, kept_rows;
    int dropoff_parts, reldrop_parts; /* parts after DropOff_Subdivision and after RelativeDropoff_Subdivision */
    int selected;                     /* entries over the cutoff: `anzahl` of both stages */
    int eligible;                     /* parts of stage 1 with more than 2 * mingroup rows (RR:3303) */
    int *dropoff_labels;              /* [rows] after UnterteilungsKomplettierung: -1 for the rows left out */
    int *reldrop_labels;              /* [rows] likewise */
    int *winner;                      /* [dropoff_parts] the variation that split the part in stage 2, -1: none */
    int *winner_cutoff;               /* [dropoff_parts] its relative cutoff c (CliqueGroup(Clique, c)), -1: none */
} pgr_subdivision;

/* Both stages on the window's Groups and the refined arrays (which are taken as they are: the refinement is not re-run, and
 * nothing is written into them -- the reference overwrites Drop_Off[] in stage 2 (RR:2912), which nothing ported reads
 * afterwards).  Stage 1 runs on the host, stage 2's votes on the device.  PWR_ERR_ARG: mincov < 0, rows / kept_rows / sc /
 * width of window and result differ, or a clique that is not -1 terminated or names a variation outside the window.
 * PWR_ERR_RANGE: more than 65535 kept rows (the kernel counts a partition's rows in 16 bits; pgr_read_window allows 30000).
 * nsig == 0 or nothing selected: every kept row gets label 0 in both outputs and the device is not touched. */
int pgr_subdivide(const pgr_window *win, const pgr_result *refined, int mincov, int device, pgr_subdivision *out);
void pgr_subdivision_free(pgr_subdivision *out);
/* Duration of the last pgr_subdivide, ms: [0] the exchange sort, [1] the rest of stage 1, [2] upload, [3] kernel, [4] apply
 * (winners' groups, splits, renumbering).  (Kept per process, not per call.) */
int pgr_last_subdivision_timing(double *ms5);

/* ---- host side, plain C (pgr_host.c) ---- */
/* DropOff_Subdivision (RR:3180-3271) with the exchange sort of RR:3199-3213 as it is (not stable: a library sort would
 * change the labels): labels[kept_rows] before UnterteilungsKomplettierung, *parts their number; ms2 (may be NULL): [0] the
 * sort, [1] the splitting loop. */
int pgr_dropoff_subdivision(const pgr_result *refined, int mingroup, int *labels, int *parts, double *ms2);
/* Unterteilungskomprimierung (RR:1823-1843): renumbers labels[n] by first appearance; returns the number of parts */
int pgr_compress_labels(int n, int *labels);
/* UnterteilungsKomplettierung (RR:1845-1865): out[rows] = the labels of the kept rows, -1 for the others */
int pgr_complete_labels(int rows, const unsigned char *kept, const int *labels, int *out);
/* Unterteilung_Rausschreiben (RR:568-585): decimal labels separated by '\n', no trailing newline */
int pgr_write_subdivision(const char *path, const int *labels, int rows);
/* The reference's file name "<stage>SubdivisionOf_<von>_<bis>_<msa>" (RR:4041-4046; stage = "Dropoff" or "RelDrop").  von
 * and bis are the ones main() printed into von_string / bis_string (RR:3962-3965): its own variables after RR:3948-3952,
 * so von = bis = -1 gives 0 and 1500000; Einlesen clips a copy of bis (RR:328), which does not reach the name.
 * PWR_ERR_RANGE if buf[n] is too small. */
int pgr_subdivision_name(char *buf, size_t n, const char *stage, int von, int bis, const char *msa);

/* ---- the k-means subdivision (RR:4064-4075) ---- */
/* Kmeans_Subdivision on the labels RelativeDropoff_Subdivision left: every part with more than 2 * mingroup rows (an
 * "eligible" part, numbered e = 0 .. eligible - 1 in ascending order of its label) gets its variables (Relative_Vars) and is
 * clustered on them (Kmeans).  Per eligible part: */
typedef struct {
    int rows, kept_rows;
    int parts_before, parts;          /* after the first and after the last Unterteilungskomprimierung (RR:3385, RR:3398) */
    int eligible;
    int *labels;                      /* [rows] after UnterteilungsKomplettierung: -1 for the rows left out */
    int *part;                        /* [eligible] the part's label after RR:3385 */
    int *part_rows;                   /* [eligible] anzahl */
    int *row_offset;                  /* [eligible + 1] into row / cluster_before / cluster_after */
    int *row;                         /* the kept-row indices I[] of each part, ascending */
    int *cluster_before;              /* Clusternumber after the assignment (RR:2706-2723) */
    int *cluster_after;               /* Clusternumber after the reassignment chain (RR:2726-2755) */
    int *varzahl;                     /* [eligible] */
    int *var_offset;                  /* [eligible + 1] into vars */
    int *vars;                        /* Vars of each part, ascending */
    long long pairs;                  /* pairs (i, j >= i + 100) evaluated by Relative_Vars, all parts */
    /* only from pgr_kmeans_subdivide_pairs: every evaluated pair, by part, then i, then j ascending */
    long long debug_pairs;
    int *pair_part, *pair_i, *pair_j; /* [debug_pairs] e, i, j */
    double *pair_z;                   /* [debug_pairs] Relative_Group_Significance(Groups[j], Groups[i], U) */
} pgr_kmeans;

/* win and refined as for pgr_subdivide (of refined only kept, maxcorrs and cutoff are read); reldrop_labels_rows[rows] =
 * pgr_subdivision.reldrop_labels (-1 for the rows left out).  The relative significance of every pair and the O(rows^2)
 * passes of Kmeans (centroids, assignment, the scores the chain reads) run on the device; the chain itself walks a
 * device-made matrix of 16-bit scores on the host.  PWR_ERR_ARG: as pgr_subdivide, or a label below -1 / a kept row labelled
 * -1.  PWR_ERR_RANGE: more than 65535 eligible parts, an eligible part with more than 65471 variables (a score would not fit
 * 16 bits), or the score matrices
 * of all eligible parts together beyond 2^28 entries (only where the chain runs: mincov > 5).  No eligible part: the device
 * is not touched and labels are the compressed input. */
int pgr_kmeans_subdivide(const pgr_window *win, const pgr_result *refined, const int *reldrop_labels_rows, int mincov, int device,
                         pgr_kmeans *out);
void pgr_kmeans_free(pgr_kmeans *out);
/* The same, and every evaluated pair's Z in out->pair_* (for tests; PWR_ERR_RANGE beyond 2^24 pairs or matrix entries) */
int pgr_kmeans_subdivide_pairs(const pgr_window *win, const pgr_result *refined, const int *reldrop_labels_rows, int mincov, int device,
                               pgr_kmeans *out);
/* Duration of the last pgr_kmeans_subdivide, ms: [0] all, [1] upload + counts |G & U|, [2] the significance kernel, [3]
 * centroids + assignment + scores, [4] the chain on the host; [5] pairs evaluated.  (Kept per process, not per call.) */
int pgr_last_kmeans_timing(double *ms6);
/* Test hooks, not product: the device's tail functions as the group refinement's and the k-means stage's files compile them,
 * arguments and refusals as pmc_tail_probe (pmc.h).  pgr_tail_probe: out[n][2] = the tail's -log10 with floor[t],
 * Group_PositiveSignificance (RR:472-488) with floor[t] (size1 = |G_i|, size2 = |G_a|).  pgr_km_tail_probe: out[n][3] =
 * hypergeometric P(schnitt), Q(schnitt - 1) (0 at schnitt = 0, RR:493), the relative significance (RR:490-504); floor is
 * not read. */
int pgr_tail_probe(int n, const int *counts, const double *floor, int device, double *out);
int pgr_km_tail_probe(int n, const int *counts, const double *floor, int device, double *out);

/* ---- host side, plain C (pgr_host.c) ---- */
/* The reassignment chain of Kmeans (RR:2726-2755), literally: scores[i * anzahl + j] = GrMatch(Centroids[j], VarSigs[i]),
 * clusternumber[anzahl] in place (entries in [0, anzahl): PWR_ERR_ARG otherwise).  mingroup <= 2: nothing moves. */
int pgr_kmeans_reassign(int anzahl, const unsigned short *scores, int mingroup, int *clusternumber);

/* ---- the whole repeat: several windows of one MSA (the reference README's `-f x y`, `-f y z`, ... and their connection) ---- */
/* The MSA resident on the device: text = rows x width characters, uploaded once.  Limits and errors as pgr_read_window;
 * PWR_ERR_NOMEM when the device (or the host) cannot hold it.  Every index into the text is 64-bit. */
typedef struct pgr_msa pgr_msa;
int pgr_msa_open(int rows, int width, const unsigned char *text, int device, pgr_msa **h);
void pgr_msa_close(pgr_msa *h);
/* Einlesen (RR:293-429) on the device copy (pgr_win_device.hip): *win and the return code are what pgr_read_window gives
 * for the same text, von and bis, bit for bit (von = bis = -1 and the clipping of bis included).  Release *win with
 * pgr_window_free. */
int pgr_msa_window(pgr_msa *h, int von, int bis, pgr_window *win);

/* One window of a resolution: what the three stages leave for [von, bis] */
typedef struct {
    int von, bis;                     /* as given: sites[p], sites[p + 1] */
    int kept_rows;
    int dropoff_parts, reldrop_parts, kmeans_parts;
    double cutoff;                    /* the one used (RR:3977) */
    int *dropoff_labels;              /* [rows] -1 for the rows left out */
    int *reldrop_labels;              /* [rows] */
    int *kmeans_labels;               /* [rows] */
} pgr_resolved_window;

typedef struct {
    int rows, nwindows;
    pgr_resolved_window *windows;     /* [nwindows] */
} pgr_resolution;

/* Window p = [sites[p], sites[p + 1]], both ends inclusive, p = 0 .. nsites - 2: every window is read on the device
 * (pgr_msa_window's kernels) and goes through the arithmetic of pgr_refine, pgr_subdivide and pgr_kmeans_subdivide.  The
 * refinement reads the sets the reader left on the device; the window is downloaded once for the host parts of the other two
 * stages, which run through their entry points above.  maxcorrs_full[width * 5], mincov and cutoff as for pgr_refine.
 * PWR_ERR_ARG: nsites < 2, sites not strictly increasing or negative; any other failure is the failing stage's code, and
 * *out is then empty. */
int pgr_msa_resolve(pgr_msa *h, const double *maxcorrs_full, int nsites, const int *sites, int mincov, double cutoff,
                    pgr_resolution *out);
void pgr_resolution_free(pgr_resolution *out);
/* Duration of the last pgr_msa_resolve and of the pgr_msa_open before it, ms: [0] the upload of the text (pgr_msa_open),
 * [1] all of pgr_msa_resolve, and summed over its windows [2] the reader kernels (with the kept-row list), [3] the download of
 * the window, [4] the refinement, [5] the subdivisions, [6] the k-means stage.  (Kept per process, not per call.) */
int pgr_last_resolve_timing(double *ms7);

/* ---- host side, plain C (pgr_host.c): the connection of the windows (SimDataAssessment.py:359-391, "SDA:") ---- */
typedef struct {
    int k_first, k_last;              /* parts of the first and of the last labelling: max label + 1 */
    double *matrix;                   /* [k_first][k_last] AllConCon after the normalisation (SDA:384-391) */
    int *best;                        /* [k_first] the first column with the largest value above 0.0 (SDA:399-405); -1: a zero row */
    double *confidence;               /* [k_first] the value there; 0.0 for a zero row */
    int *mutual;                      /* [k_first] 1: that value is also the maximum of its column */
} pgr_connection;

/* ProbabilityMatrix (SDA:359-370) between neighbours of labels[nres][rows] (-1: the row is not in that labelling), the
 * forward matrices multiplied left to right, the backward ones (of the reversed list) likewise, connection = forward x
 * transposed backward elementwise, every row divided by its sum where that is > 0 (SDA:372-391); all in doubles.  nres = 2:
 * one matrix each way.  PWR_ERR_ARG: nres < 2, rows <= 0, a label below -1, a labelling without a label >= 0. */
int pgr_connect(int nres, int rows, const int *labels, pgr_connection *out);
void pgr_connection_free(pgr_connection *out);

/* ---- per-copy consensus and resolvability on the device-resident MSA (TransposonAssessment.py, "TA:") ---- */
/* For a labelling of the rows: the symbol counts of every part in every column of the window, their consensus, and the
 * number of columns in which the consensus of two parts differ.  Symbols as base_code.h codes them (a c g t 0 .. 3, '-' and '_'
 * 4; anything else is blank and counted nowhere: counter[5] = 0, TA:90).  The parts are the labels that occur, ascending
 * (GroupMaker, TA:159-160); rows labelled -1 belong to none.  The consensus of a column is the FIRST code with the largest
 * count (np.argmax, TA:91): a beats c on a tie, any base beats '-'; where no row of the part has a symbol (depth 0) it is
 * code 0, as in the reference.  A column x is selected when max(maxcorrs_full[5x .. 5x + 4]) > cutoff (TA:263, TA:157),
 * compared on the host in doubles; maxcorrs_full = NULL selects every column of the window.  diff is Diff (TA:94-95) over the
 * selected columns -- a consensus is never blank, so a Hamming distance --, diff_all the same over all columns. */
#define PGR_CS_TILE 1024         /* window columns per work-group of the counts kernel (pgr_cons_device.hip) */
#define PGR_CS_ROWS 255          /* rows of one part per work-group (8-bit counters): a longer part is spread over several, added by atomics */
#define PGR_CS_SCRATCH_INTS (1 << 25)   /* most count entries (parts * columns * 5) held on the device at a time: a wider
                                         * window is worked through in column ranges, a whole number of tiles each */
typedef struct {
    int rows, von, bis, width;        /* window [von, bis] inclusive as elsewhere in this header; width = bis + 1 - von */
    int parts;                        /* labels that occur */
    int *part_label, *part_rows;      /* [parts] ascending labels, rows of each */
    unsigned char *consensus;         /* [parts][width] codes 0..4 */
    int *depth;                       /* [parts][width] rows of the part with a symbol there: the sum of the five counts */
    int *counts;                      /* [parts][width][5], NULL unless asked for */
    int nselected; int *selected;     /* absolute columns, ascending */
    int *diff, *diff_all;             /* [parts][parts] */
} pgr_consensus;

/* von = bis = -1: the whole width.  PWR_ERR_ARG: a label below -1, von > bis, an end outside the text, no row with a label
 * >= 0; PWR_ERR_RANGE: a label >= PGR_MAX_ROWS; PWR_ERR_NOMEM: the host cannot hold the result, or the device not even one
 * tile of columns of every part.  want_counts != 0 fills counts.  *out holds malloc'ed arrays (empty after a failure):
 * release them with pgr_consensus_free.  All results are integers and do not depend on the order of the atomics. */
int pgr_msa_consensus(pgr_msa *h, const int *labels, int von, int bis, const double *maxcorrs_full /* width*5 or NULL */,
                      double cutoff, int want_counts, pgr_consensus *out);
void pgr_consensus_free(pgr_consensus *out);
/* Duration of the last pgr_msa_consensus, ms: [0] all, [1] the sort by part and the upload of order, [2] the counts kernel,
 * [3] the consensus and diff kernels, [4] the downloads.  (Kept per process, not per call.) */
int pgr_last_consensus_timing(double *ms5);

/* ---- host side, plain C (pgr_host.c) ---- */
/* Resolvability (TA:97-119) on diff[parts][parts]: unique11[t], t = 0 .. 10, = the parts whose smallest diff to any other
 * part is > t; min_diff[parts] that smallest diff; last_diff[parts] what the reference itself returns, the diff to the LAST
 * other part visited (TA:112 appends `diff`, not `mindiff`).  PWR_ERR_ARG: fewer than two parts (the reference stops on an
 * undefined name). */
int pgr_resolvability(int parts, const int *diff, int *unique11, int *min_diff, int *last_diff);

/* ---- every row against the consensus of every part, on the device-resident MSA (pgr_assign_device.hip) ---- */
/* The reverse of pgr_msa_consensus: given the parts' consensus, which part does a row belong to?  THE REFERENCE HAS NO
 * COUNTERPART: these semantics are this project's own.
 * The window is the `width` columns from von on; codes[p][c - von] is part p's code (0 .. 4, as pgr_consensus.consensus) in
 * the absolute column c; columns[ncolumns] are the compared columns.  With base_code as in base_code.h (a c g t in either case
 * 0 .. 3, '-' and '_' 4, every other byte 5):
 *   mismatches[r][p] = the number of columns c in `columns` with base_code(text[r][c]) <= 4 and
 *                      base_code(text[r][c]) != codes[p][c - von].  A row's blank, or any other byte of code 5, is compared
 *                      nowhere.  A gap ('-' or '_') is a symbol: it matches code 4 and nothing else.
 *   compared[r]      = the number of columns c in `columns` with base_code(text[r][c]) <= 4: the same for every part.
 *   best[r]          = the part with the fewest mismatches, the lowest index among equals; second[r] the same rule over the
 *                      other parts; best_mismatches[r] and second_mismatches[r] their counts.  Where compared[r] == 0 both
 *                      are -1 and both counts 0; where parts == 1, second[r] is -1 and second_mismatches[r] is 0.
 * best and second are part INDICES 0 .. parts - 1, not labels.  Everything is an integer, computed without atomics: no result
 * depends on an order. */
#define PGR_AS_SCRATCH_BYTES (64 << 20)   /* most device scratch per range of rows (planes + mismatch matrix) */
#define PGR_AS_TILE 8            /* parts per work-group of the distance kernels (row_planes.h: k_as_dist, k_st_dist) */

typedef struct {
    int rows, parts, ncolumns;
    int *compared;            /* [rows] columns of `columns` at which the row has a symbol (base_code 0..4) */
    int *best, *second;       /* [rows] part INDEX 0..parts-1, or -1 */
    int *best_mismatches;     /* [rows] */
    int *second_mismatches;   /* [rows] */
    int *mismatches;          /* [rows][parts], or NULL unless asked for */
} pgr_assignment;

/* The rows go through the device in ranges of at most PGR_AS_SCRATCH_BYTES / (32 * ceil(ncolumns / 64) + 4 * parts) rows (one
 * at least; 32 bytes per row and 64 columns of bit planes, 4 per row and part of the matrix), halved while the device refuses.
 * PWR_ERR_ARG: a null pointer; parts < 1; width < 1; a window outside the text; a code above 4; ncolumns < 1; columns that do
 * not ascend strictly or lie outside [von, von + width - 1] -- all refused before the device is touched.  PWR_ERR_RANGE:
 * parts > PGR_MAX_ROWS.  PWR_ERR_NOMEM: the host cannot hold the result, or the device not even one row.  want_matrix != 0
 * fills mismatches.  *out is zeroed first and holds malloc'ed arrays (empty after a failure): release them with
 * pgr_assignment_free. */
int  pgr_msa_assign(pgr_msa *h, int parts, int von, int width, const unsigned char *codes /* [parts][width], 0..4 */,
                    int ncolumns, const int *columns /* absolute, strictly ascending, inside [von, von+width-1] */,
                    int want_matrix, pgr_assignment *out);
void pgr_assignment_free(pgr_assignment *out);
/* Duration of the last pgr_msa_assign, ms: [0] all, [1] checks, part planes, upload and allocation, [2] the planes kernel,
 * [3] the distance and best kernels, [4] the downloads.  (Kept per process, not per call.) */
int  pgr_last_assign_timing(double *ms5);

/* ---- a labelling settled on the device: consensus and assignment iterated (pgr_settle_device.hip) ---- */
/* The two calls above are the halves of one loop; this entry runs it on the device.  THE REFERENCE HAS NO COUNTERPART.  The
 * result is defined by the composition of the public calls (resolution.consensus / assign / Assignment.labels are the Python
 * names of the steps), everything an integer:
 *   lab = labels; history = []; last = none; stop = MAX_ITER
 *   for it in 0 .. max_iter - 1:
 *       con = pgr_msa_consensus(lab, von, bis, maxcorrs_full, cutoff)
 *       columns = the candidates at which every part of con has depth >= min_depth; none: stop = NO_COLUMN, break
 *       a = pgr_msa_assign(con.consensus, columns)
 *       new[r] = con.part_label[a.best[r]] where a.best[r] >= 0, a.compared[r] >= min_compared and (a.second[r] == -1 or
 *                a.second_mismatches[r] - a.best_mismatches[r] >= min_margin), else -1; with hold, labels[r] -- the INITIAL
 *                label -- wherever that is >= 0
 *       changed = the rows with new != lab; history += (changed, con.parts, the number of columns); last = a
 *       changed == 0: stop = CONVERGED, break;  no new[r] >= 0: stop = EMPTY, break (lab stays);  lab = new
 * The candidates are con.selected (every column of the window with all_columns != 0, or maxcorrs_full = NULL) and are fixed for
 * the call; which of them are compared changes with the depths.  The parts of an iteration are the labels that occur in lab
 * then, ascending, as a fresh pgr_msa_consensus numbers them: a label no row holds any more is no part, constrains no column,
 * and no row can join it (with hold the initial labels never die).  best and second are indices among the parts of the LAST
 * iteration -- the one whose assignment made the labels returned; with EMPTY the one that emptied the labelling --, part_label
 * [parts] their labels, columns[ncolumns] its compared columns.  NO_COLUMN in iteration 0 has no last iteration: parts,
 * ncolumns and iterations are 0 and every array but labels is NULL, the three histories included. */
#define PGR_ST_CONVERGED 0       /* an iteration moved no row */
#define PGR_ST_MAX_ITER 1        /* max_iter iterations, the last of which still moved rows */
#define PGR_ST_EMPTY 2           /* an iteration left no row with a label: the labelling before it is returned */
#define PGR_ST_NO_COLUMN 3       /* no candidate column at which every part has depth >= min_depth */

typedef struct {
    int rows, iterations, stop, parts;        /* iterations = entries of the history; stop: PGR_ST_*; parts of the last iteration */
    int *part_label;                          /* [parts] */
    int *labels;                              /* [rows] the settled labelling */
    int *changed, *parts_at, *ncolumns_at;    /* [iterations] rows moved, parts, compared columns of every iteration */
    int ncolumns; int *columns;               /* the compared columns of the last iteration: absolute, ascending */
    int *compared, *best, *second, *best_mismatches, *second_mismatches;   /* [rows] as pgr_assignment, of the last iteration */
} pgr_settlement;

/* The rows' bit planes over the candidates stay on the device for the whole call: 32 * ceil(candidates / 64) * rows bytes, and
 * 4 * rows * parts bytes of mismatches; PWR_ERR_NOMEM if the device refuses (there are no ranges).  Argument errors as
 * pgr_msa_consensus (PWR_ERR_ARG: a null pointer, a label below -1, von > bis, an end outside the text, no label >= 0;
 * PWR_ERR_RANGE: a label >= PGR_MAX_ROWS) and PWR_ERR_ARG for max_iter < 1, min_depth < 1, min_compared < 0, min_margin < 0 --
 * all refused before the device is touched.  *out is zeroed first and holds malloc'ed arrays (empty after a failure): release
 * them with pgr_settlement_free.  Sums of integers only: no result depends on the order of the atomics. */
int  pgr_msa_settle(pgr_msa *h, const int *labels, int von, int bis, const double *maxcorrs_full /* width*5 or NULL */, double cutoff,
                    int min_depth, int all_columns, int min_compared, int min_margin, int hold, int max_iter, pgr_settlement *out);
void pgr_settlement_free(pgr_settlement *out);
/* Duration of the last pgr_msa_settle, ms: [0] all, [1] checks, candidates, allocation and upload, [2] the planes kernel,
 * [3] the iterations in total, [4] the downloads.  (Kept per process, not per call.) */
int  pgr_last_settle_timing(double *ms5);

/* ---- rows that change copy: every row against every part per segment, and its best crossover (pgr_cross_device.hip) ---- */
/* pgr_msa_assign compares a row with every part over all compared columns at once: a row that follows part A through the first
 * segments and part B through the rest is a poor match of either.  THE REFERENCE HAS NO COUNTERPART: these semantics are this
 * project's own.  h, parts, von, width, codes, ncolumns and columns as for pgr_msa_assign, base_code as there.  seg_end[nseg]
 * cuts columns[] into consecutive segments: segment s holds the entries [seg_end[s - 1], seg_end[s]) of columns[], with
 * seg_end[-1] = 0; seg_end ascends strictly and seg_end[nseg - 1] == ncolumns, so no segment is empty.
 *   seg_mismatches[r][s][p], seg_compared[r][s] = what pgr_msa_assign defines as mismatches[r][p] and compared[r], over the
 *                      columns of segment s alone.
 *   compared, best, second, best_mismatches, second_mismatches = exactly what pgr_msa_assign returns for the same codes and
 *                      columns: the one-copy explanation of the row.
 *   seg_best[r][s]   = the part with the fewest mismatches in segment s, the lowest index among equals; -1 where
 *                      seg_compared[r][s] == 0.
 *   the crossover of row r, its two-copy explanation: a split k in 1 .. nseg - 1 is admissible when the row has at least
 *                      min_side compared columns in the segments < k and at least min_side in the segments >= k.  For an
 *                      admissible k and parts a != b, total(k, a, b) = the sum over s < k of seg_mismatches[r][s][a] + the sum
 *                      over s >= k of seg_mismatches[r][s][b].  The crossover is the lexicographically smallest (total, k, a, b):
 *                      cross_split[r] = k, cross_left[r] = a, cross_right[r] = b (part INDICES), cross_mismatches[r] = total,
 *                      cross_left_compared[r] = the row's compared columns in the segments < k.  Where nseg < 2, parts < 2 or no
 *                      split is admissible the three indices are -1 and the two counts 0.
 * A split lies between two segments, never inside one (use finer segments), and a row has one crossover.  Everything is an
 * integer, computed without atomics: no result depends on an order. */
#define PGR_CX_MAX_SEGMENTS 1024 /* most segments of one call */

typedef struct {
    int rows, parts, ncolumns, nseg;
    int *compared, *best, *second, *best_mismatches, *second_mismatches;   /* [rows] as pgr_assignment */
    int *seg_compared;        /* [rows][nseg] */
    int *seg_best;            /* [rows][nseg] part INDEX, or -1 */
    int *cross_split;         /* [rows] 1 .. nseg-1, or -1 */
    int *cross_left, *cross_right;   /* [rows] part INDEX, or -1 */
    int *cross_mismatches;    /* [rows] */
    int *cross_left_compared; /* [rows] */
    int *seg_mismatches;      /* [rows][nseg][parts], or NULL unless asked for */
} pgr_crossovers;

/* Every segment is padded to whole words of 64 columns on the device (W = the sum over the segments of ceil(columns of the
 * segment / 64)); the rows go through in ranges of at most PGR_AS_SCRATCH_BYTES / (32 * W + 4 * nseg * parts + 8 * nseg + 40)
 * rows (one at least: the bit planes, the matrix and the per-row results), halved while the device refuses.  Errors as
 * pgr_msa_assign (PWR_ERR_ARG: a null pointer, seg_end included; parts < 1; width < 1; a window outside the text; a code above 4;
 * ncolumns < 1; columns that do not ascend strictly or lie outside the window; PWR_ERR_RANGE: parts > PGR_MAX_ROWS), and
 * PWR_ERR_ARG for nseg < 1, a seg_end that does not ascend strictly from above 0 or does not end at ncolumns, and min_side < 1;
 * PWR_ERR_RANGE for nseg > PGR_CX_MAX_SEGMENTS -- all refused before the device is touched.  want_matrix != 0 fills
 * seg_mismatches.  *out is zeroed first and holds malloc'ed arrays (empty after a failure): release them with
 * pgr_crossovers_free. */
int  pgr_msa_crossovers(pgr_msa *h, int parts, int von, int width, const unsigned char *codes /* [parts][width], 0..4 */,
                        int ncolumns, const int *columns, int nseg, const int *seg_end /* [nseg] */, int min_side, int want_matrix,
                        pgr_crossovers *out);
void pgr_crossovers_free(pgr_crossovers *out);
/* Duration of the last pgr_msa_crossovers, ms: [0] all, [1] checks, padding, part planes, upload and allocation, [2] the planes
 * kernel, [3] the segment distances, [4] the crossover and best kernels, [5] the downloads.  (Kept per process, not per call.) */
int  pgr_last_crossover_timing(double *ms6);

/* ---- host side, plain C (pgr_host.c): the windows' labellings threaded into whole copies ---- */
/* The discrete counterpart of pgr_connect, integers only.  labels[nres][rows] as pgr_connect takes them (-1: the row is not in
 * that labelling; flank labellings may stand in front and behind).  For neighbours i, i + 1: C_i[a][b] = the rows labelled
 * a >= 0 in i and b >= 0 in i + 1.  (i, a) and (i + 1, b) are LINKED when C_i[a][b] > 0, b is the first largest of row a of C_i
 * and a is the first largest of column b.  A thread is a maximal chain of links: every label that occurs in a labelling lies on
 * exactly one thread, possibly alone.  Threads are numbered by (labelling, label) of their first element, ascending. */
typedef struct {
    int nres, rows, nthreads;
    int *first, *last;        /* [nthreads] the labellings in which the thread begins and ends */
    int *offset;              /* [nres + 1] offset[0] = 0, offset[i + 1] = offset[i] + k_i, k_i = (the largest label of labelling i) + 1 */
    int *thread_of;           /* [offset[nres]] thread_of[offset[i] + label]; -1: the label does not occur in labelling i */
    int *row_thread;          /* [rows] the thread common to all of the row's labels >= 0; -1: it has none, or they disagree */
    int *row_conflict;        /* [rows] 1 exactly where they disagree */
} pgr_threads;

/* Errors as pgr_connect (PWR_ERR_ARG: a null pointer, nres < 2, rows <= 0, a label below -1, a labelling without a label >= 0).
 * *out is zeroed first and holds malloc'ed arrays (empty after a failure): release them with pgr_threads_free. */
int  pgr_thread(int nres, int rows, const int *labels, pgr_threads *out);
void pgr_threads_free(pgr_threads *out);

#ifdef __cplusplus
}
#endif
#endif /* PGR_H */
