/*
 * pfl.h -- C ABI of the flank labellings (part of libpwr.so): which unique sequence lies left and right of every row of the
 * MSA, found from the reads alone.  pgr_connect takes such labellings "in front and behind, as SDA:375 puts them"; the
 * reference (SimDataAssessment.py, "SDA:") takes them from the simulator's ground truth (SDA:226-245, Read2Copy of the read
 * that holds the neighbouring piece).  What follows has no counterpart there: the semantics are this project's own.
 *
 * ---- which piece is a row's flank (pfl_neighbours) ----
 * Pieces are numbered as Seq.fasta holds them; piece_read[k] is the read of piece k (ReadSeqInfo, prc_write_info's format),
 * cls[k] its SeqClass letter ('r': it became an MSA row), strand[k] its line of InitialAligner's -b file (1: '-', the row
 * is the piece's reverse complement; NULL: all forward).  MSA row t is the t-th piece of class 'r', say piece k.  The piece
 * beside it, k + 1 or k - 1, is its flank if it exists, lies in the same read and is not of class 'r' (SDA:229, SDA:237).
 *
 *     row strand   flank                           piece   how it is read               mode
 *     forward      right                           k + 1   first base to last           0
 *     forward      left                            k - 1   last base to first           1
 *     reverse      right (template orientation)    k - 1   backwards and complemented   3
 *     reverse      left                            k + 1   forwards and complemented    2
 *
 * Mode bit 0: walk the piece from its last base to its first; bit 1: complement every base (a<->t, c<->g).  The piece read
 * this way is the flank's ANCHORED SEQUENCE: it starts at the repeat boundary and runs away from it.  No reverse complement
 * is made or uploaded anywhere: a flank carries its mode and the kernel walks accordingly.
 *
 * ---- distance of two flanks (pfl_distances), integers only ----
 * reach in 1 .. PFL_MAX_REACH, min_len >= 1.  With len_k the length of flank k's piece, a_k = min(len_k, reach).  A flank
 * with len_k < min_len is SHORT: its row and column of the matrix are -1 (the diagonal entry too) and its label is -1.  The
 * others are ordered by (a_k, k); for a pair of which i comes first in that order
 *     m = a_i,
 *     P = the first m bases of i's anchored sequence,
 *     T = the first min(len_j, m + m / 4) bases of j's anchored sequence (|T| >= m),
 *     D(0, y) = y, D(x, 0) = x, unit costs for substitution, insertion and deletion,
 *     d = min over 0 <= y <= |T| of D(m, y)        (both start at the boundary; where P ends in T is free),
 *     dist[i][j] = dist[j][i] = d, and dist[i][i] = 0.
 * The pattern is always the shorter of the two, so the relation is symmetric by construction.
 *
 * ---- clustering (pfl_cluster), host only ----
 * i and j (neither short) are joined iff 1000 * d <= max_permille * min(a_i, a_j).  The labels are the connected components
 * (single linkage); a component with fewer than min_size flanks gets -1, the others are numbered from 0 in the order of
 * their lowest flank index.  max_permille has no default: it depends on the reads' error rate (DESIGN 23 has the table).
 *
 * Error codes are those of pwr.h.
 */
#ifndef PFL_H
#define PFL_H

#include <stdio.h>

#include "pwr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFL_MAX_REACH 512        /* 16 words of 32 pattern rows in a lane's registers */
#define PFL_MAX_FLANKS 30000     /* flanks of one call (PGR_MAX_ROWS: there are no more rows) */

typedef struct pfl_ctx pfl_ctx;

/* The context owns the device buffers of the last call (the packed flanks, the tiles, the distances); they are reused and
 * grown by the next call and freed by pfl_destroy, so at most one call's pieces are resident per context.  The device is
 * first touched by the first call that has a pair to compute: creating a context, and every refusal below, needs no GPU. */
int pfl_create(pfl_ctx **out, int device);
void pfl_destroy(pfl_ctx *ctx);

/* The rule above, host only.  cls: npieces SeqClass letters; strand: npieces bytes or NULL.  Row t < *nrows: row_piece[t],
 * left_piece[t] / right_piece[t] (-1: no flank) and left_mode[t] / right_mode[t] (the mode the flank would have, also where
 * there is none).  Every output has room for npieces entries. */
int pfl_neighbours(int npieces, const int *piece_read, const char *cls, const unsigned char *strand, int *nrows, int *row_piece,
                   int *left_piece, int *left_mode, int *right_piece, int *right_mode);

/* The distances of n flanks: flank k is piece piece[k] (bases[off[p] .. off[p + 1]), acgt in either case) read in mode
 * mode[k].  len_out[k] = len_k; dist_out is the n x n matrix above.  Only the bases a distance can reach -- the
 * min(len_k, reach + reach / 4) nearest to the boundary -- go to the device, once per flank, packed into one upload; pairs
 * copy nothing.  A byte outside acgtACGT anywhere in a listed piece -> PWR_ERR_INPUT (pieces that are not listed are not
 * looked at); reach outside 1 .. PFL_MAX_REACH, min_len < 1 or n > PFL_MAX_FLANKS -> PWR_ERR_RANGE; a negative piece, a mode
 * outside 0 .. 3 or descending offsets -> PWR_ERR_ARG.  n == 0 is valid, and fewer than two flanks of min_len make no
 * device call. */
int pfl_distances(pfl_ctx *ctx, int n, const char *bases, const long long *off, const int *piece, const int *mode, int reach,
                  int min_len, int *len_out, int *dist_out);

/* Single linkage on dist (n x n, as pfl_distances wrote it; dist[i][i] < 0 marks a short flank) with a[k] = min(len_k, reach).
 * Host only.  max_permille < 0 or min_size < 1 -> PWR_ERR_ARG. */
int pfl_cluster(int n, const int *a, const int *dist, int max_permille, int min_size, int *label_out);

/* Pattern x text cells of the DP tables the calls so far stand for (m * |T| per pair) and the summed kernel time, ms. */
int pfl_get_stats(pfl_ctx *ctx, unsigned long long *cells, double *kernel_ms);

/* The chain for one repeat: pfl_neighbours, then per side pfl_distances and pfl_cluster over the rows that have a flank
 * there.  left[t] / right[t] (room for npieces each) = the label of row t's flank or -1: FlankingLeft and FlankingRight in
 * the shape pgr_connect takes. */
int pfl_labels(pfl_ctx *ctx, int npieces, const char *bases, const long long *off, const int *piece_read, const char *cls,
               const unsigned char *strand, int max_permille, int reach, int min_len, int min_size, int *nrows, int *left,
               int *right);

/* ---- files, plain C ---- */
/* ReadSeqInfo (prc_write_info: one line per read, its piece numbers each followed by a space): *piece_read (malloc'ed,
 * pfl_free) gets the read of every piece.  Numbers that do not count up from 0 -> PWR_ERR_INPUT. */
int pfl_read_info(const char *path, int *npieces, int **piece_read);
void pfl_free(void *p);
/* One integer per line, as SDA:248-256 would write <dataset>_FlankingLeft. */
int pfl_write_labels(const char *path, int n, const int *labels);
/* The drop-in FlankClusterer: Seq.fasta (pia_read_fasta), ReadSeqInfo, SeqClass (one letter per line), strand_path (one +
 * or - per line; NULL: all forward) -> left_path and right_path through pfl_labels.  Returns the process exit code.
 * ReadCutter, like the reference, never sets the cut count of the last record it writes (prc_run_files: "Cutting_Number[n-1]
 * is never set"), so its ReadSeqInfo lists one piece for that read whatever Seq.fasta holds: where the file lists fewer
 * pieces than Seq.fasta has, the pieces past the listed ones are taken as the last listed read's.  More listed pieces than
 * Seq.fasta holds is an error. */
int pfl_run_files(const char *seq_path, const char *info_path, const char *class_path, const char *strand_path, int max_permille,
                  int reach, int min_len, int min_size, const char *left_path, const char *right_path, int device, FILE *log);

#ifdef __cplusplus
}
#endif
#endif /* PFL_H */
