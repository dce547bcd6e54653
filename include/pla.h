/*
 * pla.h -- C ABI of the locus anchorer (part of libpwr.so): where in an assembly the copies of a resolved repeat belong.
 * pipeline.loci / resolution.write_loci end with "left flank + copy + right flank" per copy; here the bases of every flank
 * nearest to the repeat boundary are looked up in the contigs of an assembly, in both orientations, and from the hits follow
 * the placement of every locus and the patched contigs.  The reference has no counterpart: the semantics are this project's
 * own, everything is an integer, and a device result equals tests/la_checker.py exactly.
 *
 * ---- the text ----
 * nc contigs; contig c is t[0 .. L_c) = bases[off[c] .. off[c + 1]).  a c g t in either case code as 0 1 2 3, every other byte
 * (N, IUPAC, anything) as 4.  Code 4 matches no pattern base and is never dropped: coordinates are the file's.
 *
 * ---- a pattern ----
 * A pattern is given as an ANCHORED SEQUENCE A (pfl.h: what pfl_consensus_result.seq holds -- first base at the repeat
 * boundary, running away from the repeat) with its side (0 left, 1 right).  reach in 1 .. PLA_MAX_REACH, min_len >= 1,
 * m = min(|A|, reach); the searched rows are Q[x] = A[m - 1 - x], x = 0 .. m - 1: Q ends with the base at the boundary.  A
 * pattern with |A| < min_len is SHORT and has no hits.
 *
 * ---- the walk ----
 * Each pattern is searched in two orientations o (0: +, 1: -).  Job (pattern, o) walks a contig as W[0 .. L_c): backwards,
 * W[y] = t[L_c - 1 - y], iff side != o, else forwards, W[y] = t[y]; and with every base complemented (code 3 - code for the
 * codes below 4) iff o == 1.
 *     left  +  forwards             left  -  backwards, complemented
 *     right +  backwards            right -  forwards, complemented
 * No reverse complement is made or uploaded: a job carries its two bits.
 *
 * ---- the table ----
 * D(0, y) = 0 (the pattern may begin anywhere), D(x, 0) = x, unit costs for substitution, insertion and deletion;
 * k = floor(max_permille * m / 1000), max_permille in 0 .. 500 and without a default.
 *
 * ---- a hit ----
 * A maximal run of walk columns y1 .. y2 within 1 .. L_c with D(m, y) <= k.  distance = the run's minimum, y* = the smallest y
 * of the run that holds it.  The boundary coordinate of a column is b(y) = y on a forward walk and L_c - y on a backward one:
 * the number of contig bases in front of the boundary.  The flank lies on the side the walk came from, the repeat begins on
 * the other.  A hit reports pattern, orientation, contig, boundary = b(y*), lo = min(b(y1), b(y2)), hi = max(b(y1), b(y2)) and
 * distance; hits are sorted by (pattern, orientation, contig, boundary).  How the device cuts the walk into chunks does not
 * show in the result.
 *
 * ---- placement of a locus (pla_place), host only ----
 * A locus has a left and a right pattern (or none on a side: -1).  It takes the hits of both, in both orientations and on all
 * contigs.  max_span has no default.  In this precedence:
 *     PLA_NONE          no hit on either side
 *     PLA_AMBIGUOUS     a side has two or more hits: that flank is not unique in this assembly
 *     PLA_LEFT_ONLY     exactly one hit on the left and none on the right;  PLA_RIGHT_ONLY the other way round
 *   and with exactly one hit on each side, bL and bR being their boundaries,
 *     PLA_PLACED        same contig, same orientation and span in 0 .. max_span, span = bR - bL for + and bL - bR for -;
 *                       the interval is [min(bL, bR), max(bL, bR))
 *     PLA_BRIDGE        different contigs: the assembly broke at the repeat
 *     PLA_INCONSISTENT  same contig, but different orientations or a span outside 0 .. max_span
 *   and at the end
 *     PLA_CONFLICT      two PLACED loci on one contig whose intervals overlap (lo_a < hi_b and lo_b < hi_a) both become
 *                       CONFLICT; intervals that only touch do not.
 *
 * Error codes are those of pwr.h.
 */
#ifndef PLA_H
#define PLA_H

#include <stdio.h>

#include "pwr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PLA_MAX_REACH 512        /* 16 words of 32 pattern rows in a lane's registers */
#define PLA_MAX_HITS (1 << 22)   /* hits of one call */
#define PLA_MAX_PATTERNS 65536   /* patterns of one call */
#define PLA_RUN_CAP 4            /* runs a chunk has room for in the first pass; a chunk with more is run again with room */

enum { PLA_NONE = 0, PLA_AMBIGUOUS, PLA_LEFT_ONLY, PLA_RIGHT_ONLY, PLA_PLACED, PLA_BRIDGE, PLA_INCONSISTENT, PLA_CONFLICT };

typedef struct pla_ctx pla_ctx;

typedef struct pla_hits {
    int n;
    int *pattern, *orientation, *contig, *boundary, *lo, *hi, *distance;   /* [n] each */
} pla_hits;

/* Creating a context needs no GPU; the device is first touched by pla_open_text. */
int pla_create(pla_ctx **out, int device);
void pla_destroy(pla_ctx *ctx);

/* Puts the contigs on the device, once: they stay for any number of searches until pla_close_text, the next pla_open_text
 * (which replaces them) or pla_destroy.  Null pointers, nc < 0 or descending offsets -> PWR_ERR_ARG; a contig of more than
 * 2^31 - 1 bases -> PWR_ERR_RANGE; both before the device is touched.  nc == 0 and empty contigs are valid. */
int pla_open_text(pla_ctx *ctx, int nc, const char *bases, const long long *off);
void pla_close_text(pla_ctx *ctx);

/* "chunk": the walk columns a lane owns, a multiple of 4 in 32 .. 65536 (default 2048); a test hook and a tuning knob.  Any
 * other name -> PWR_ERR_ARG, any other value -> PWR_ERR_RANGE. */
int pla_set_option(pla_ctx *ctx, const char *name, long long value);

/* The search above of np patterns, pattern p being anchored[aoff[p] .. aoff[p + 1]) with side[p].  *out is zeroed first, filled
 * on success (free it with pla_hits_free) and left zeroed on failure.  Refusals, in this order and all before the device is
 * touched: null pointers, np < 0, a side outside 0 / 1 or descending offsets -> PWR_ERR_ARG; reach outside 1 .. PLA_MAX_REACH,
 * max_permille outside 0 .. 500, min_len < 1 or np > PLA_MAX_PATTERNS -> PWR_ERR_RANGE; a pattern byte outside acgtACGT (in
 * any pattern, short or not, over its whole length) -> PWR_ERR_INPUT; no text open -> PWR_ERR_UNSUPPORTED.  More than
 * PLA_MAX_HITS hits -> PWR_ERR_RANGE. */
int pla_search(pla_ctx *ctx, int np, const char *anchored, const long long *aoff, const int *side, int reach, int min_len,
               int max_permille, pla_hits *out);
void pla_hits_free(pla_hits *h);

/* Cells (m x the walked columns of every job, the warm-up of the chunks not counted) and the summed time of k_la_search, ms. */
int pla_get_stats(pla_ctx *ctx, unsigned long long *cells, double *kernel_ms);

/* ---- host only, plain C (pla_host.c): usable without a GPU ---- */
typedef struct pla_contigs {
    int nc;
    char **name;                 /* [nc] the first word after '>' (may be empty) */
    long long *off;              /* [nc + 1] */
    char *bases;                 /* every sequence byte of the file, acgtACGT kept as they are, anything else as 'n' */
} pla_contigs;

/* A FASTA: a record begins with '>', its name is the first word behind it, its sequence may span lines (line ends and blanks
 * are no sequence bytes).  Sequence before the first '>' -> PWR_ERR_INPUT; a file that cannot be opened -> PWR_ERR_IO. */
int pla_read_contigs(const char *path, pla_contigs *out);
void pla_contigs_free(pla_contigs *c);

typedef struct pla_loci {
    int n;
    char **name;                 /* [n] the first word of the header: <name>_locus<thread> */
    int *left_len, *copy_len, *right_len;
    long long *off;              /* [n + 1]: locus i is seq[off[i] .. off[i + 1]) = left + copy + right, template orientation */
    char *seq;
    /* the 2 n patterns: 2 i is locus i's left flank (side 0: its left part reversed), 2 i + 1 its right (side 1: as it is);
     * a side of 0 bases is an empty pattern, which is short at every min_len */
    long long *aoff;             /* [2 n + 1] */
    char *anchored;
    int *side;                   /* [2 n] */
} pla_loci;

/* What resolution.write_loci writes: ">name left=<L>:<bases> copy=<bases> right=<R>:<bases> ..." and the sequence on one
 * line.  A header without the three fields, or a sequence whose length is not their sum -> PWR_ERR_INPUT. */
int pla_read_loci(const char *path, pla_loci *out);
void pla_loci_free(pla_loci *l);

typedef struct pla_placement {
    int status;                  /* PLA_* */
    int left_hits, right_hits;   /* how many hits the two patterns have */
    /* of a side with exactly one hit, else -1: */
    int left_contig, left_orientation, left_boundary, left_distance;
    int right_contig, right_orientation, right_boundary, right_distance;
    int lo, hi;                  /* [lo, hi): both hits on one contig, else -1 */
    int has_span, span;          /* both hits on one contig in one orientation: has_span = 1 and the span, else 0 and 0 */
} pla_placement;

/* The rule above for nloci loci, locus i having the patterns left_pattern[i] and right_pattern[i] (-1: none) of `hits`.
 * max_span < 0 or null pointers -> PWR_ERR_ARG. */
int pla_place(int nloci, const int *left_pattern, const int *right_pattern, const pla_hits *hits, int max_span, pla_placement *out);
const char *pla_status_name(int status);

/* One line per locus, tab-separated: name, status, left contig, right contig, left orientation, right orientation, left
 * boundary, right boundary, lo, hi, span, left distance, right distance; "-" where a field does not exist. */
int pla_write_placements(const char *path, int nloci, const char *const *name, const pla_placement *p, const pla_contigs *contigs);

/* Every contig as ">name patched=<n>" and its sequence on one line.  Every PLACED interval is replaced by that locus's copy,
 * copies[coff[i] .. coff[i + 1]), reverse-complemented where the orientation is -; everything else is byte for byte as read.
 * The intervals of one contig are taken by (lo, hi, locus).  Bridges are reported, not joined. */
int pla_write_patched(const char *path, const pla_contigs *contigs, int nloci, const pla_placement *p, const char *copies,
                      const long long *coff);

/* The drop-in LocusAnchorer: loci (pla_read_loci) and assembly (pla_read_contigs) -> <prefix>_Anchors (one line per hit: locus
 * name, side, orientation, contig, boundary, lo, hi, distance), <prefix>_Placements and <prefix>_Patched.fasta.  Returns the
 * process exit code. */
int pla_run_files(const char *loci_path, const char *assembly_path, int max_permille, int max_span, int reach, int min_len,
                  const char *prefix, int device, FILE *log);

#ifdef __cplusplus
}
#endif
#endif /* PLA_H */
