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
 * ---- placement of a member against a backbone (pfl_place), integers only ----
 * block: a multiple of 32 in 32 .. PFL_MAX_REACH; extent in block .. PFL_MAX_EXTENT; max_permille >= 0 (no default).  A
 * BACKBONE is a plain sequence B, first base at the boundary.  Only its first nb = floor(min(|B|, extent) / block) blocks of
 * `block` bases are used; a partial last block is dropped.  A MEMBER M is a flank's anchored sequence, its whole length.  It
 * starts with the cursor s = 0, and for b = 0 .. nb - 1:
 *     if |M| - s < block, the member stops;
 *     P = block b of B (m = block), T = M[s : s + min(|M| - s, m + m / 4)], D as above (D(0,y) = y, D(x,0) = x, unit costs);
 *     y* = the SMALLEST y in 0 .. |T| at which D(m, y) is minimal, d = D(m, y*);
 *     if 1000 * d > max_permille * m, the member stops and casts no vote in this block;
 *     otherwise the path is traced back from (m, y*) to (0, 0), at (x, y) taking
 *         1. up        if x > 0 and D(x,y) = D(x-1,y) + 1      (the member lacks backbone base x - 1),
 *         2. left      if y > 0 and D(x,y) = D(x,y-1) + 1      (member base y - 1 is inserted),
 *         3. diagonal  otherwise,
 *     and s += y*.
 * With "up, then left, else diagonal" the gaps of equal-cost runs end up at the same end for every member, and only the +1
 * halves of the vertical and horizontal deltas are needed.  Per member and used backbone position i the result is one byte
 * ops[i]:
 *     low nibble   0 .. 3: the member's base (a c g t) on a diagonal step; 4: an up step (a gap); 15: no vote;
 *     high nibble  0, or 1 + the code of the FIRST member base of a run of left steps that directly follows position i.
 * Left steps at x = 0, in front of a block's first base, vote for nothing: an insertion between two blocks, or in front of
 * the backbone, is never seen.  This blind spot of one slot per block is part of the definition.  Also per member: the
 * blocks it voted in, the bases it consumed (s at the end) and the sum of its d.
 *
 * ---- votes and call ----
 * voters[i] = the members with a vote at i.  The symbol at i is the first largest of the counts of a, c, g, t, gap, in that
 * order; a gap emits nothing.  After it, if 2 * (members with an insertion after i) > voters[i], the first largest inserted
 * base (a, c, g, t in that order) is emitted too.  The consensus ends in front of the first i with voters[i] < min_depth
 * (min_depth >= 1), and every emitted base carries voters[i] as its depth.
 *
 * ---- consensus of every cluster (pfl_consensus) ----
 * For every label >= 0 among the flanks, ascending, the members are its flanks of at least `block` bases; a label of -1 is
 * ignored.  Round 1's backbone is the longest member's anchored sequence (ties: the lowest flank index); it is itself a
 * member and votes through its own alignment.  Round r + 1's backbone is round r's consensus, rounds >= 1.  A consensus
 * shorter than `block` is the result, and that cluster's rounds stop.  A cluster without a member gets an empty consensus
 * and backbone -1.  The consensus ends on a whole block of its backbone, so each round can lose up to block - 1 bases.
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
#define PFL_MAX_EXTENT 8192      /* backbone bases a placement uses at most */

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

/* Every member against its backbone.  Flank k is given as in pfl_distances and belongs to backbone cluster[k] in 0 .. nb - 1,
 * or to none (-1: it is not placed).  Backbone j is bb_bases[bb_off[j] .. bb_off[j + 1]), acgt in either case.  Of a member
 * the min(len_k, extent + extent / 4) bases nearest to the boundary go to the device (no placement reaches further), once.
 * ops[k * stride + i] is the byte above for i below the used bases of k's backbone and 15 for every other i < stride;
 * blocks[k], used[k], dist[k] as above (0 for a flank that is not placed).  block, extent, n or nb out of range, or stride
 * below the used bases of the longest backbone -> PWR_ERR_RANGE; null pointers, bad modes, pieces or clusters, descending
 * offsets or max_permille < 0 -> PWR_ERR_ARG; a byte outside acgtACGT in a listed piece or in a backbone -> PWR_ERR_INPUT.
 * All of these are found before the device is touched.  The traceback keeps 2 * (block / 32) * 4 * (block + block / 4) bytes
 * per member in flight in a scratch buffer of the context; where that would pass the context's limit, or the device refuses
 * it, the members go in ranges. */
int pfl_place(pfl_ctx *ctx, int n, const char *bases, const long long *off, const int *piece, const int *mode, const int *cluster,
              int nb, const char *bb_bases, const long long *bb_off, int block, int extent, int max_permille, unsigned char *ops,
              long long stride, int *blocks, int *used, int *dist);

/* The scratch a placement may take, in bytes (0 or less: the default, 1 GiB).  One tile of 64 members is always taken. */
int pfl_set_scratch_limit(pfl_ctx *ctx, long long bytes);

/* Cells (block * (block + block / 4) per member and block it voted in: the columns every lane steps) and the summed times of
 * k_fl_place and k_fl_votes, ms, so far. */
int pfl_get_place_stats(pfl_ctx *ctx, unsigned long long *cells, double *place_ms, double *votes_ms);

typedef struct pfl_consensus_result {
    int nclusters;               /* the labels >= 0 that occur */
    int *label;                  /* [nclusters] ascending */
    int *members;                /* [nclusters] flanks of the label with at least `block` bases */
    int *backbone;               /* [nclusters] the flank index of round 1's backbone, or -1 */
    long long *off;              /* [nclusters + 1]: cluster j's consensus is seq[off[j] .. off[j + 1]) */
    char *seq;                   /* lower-case acgt, anchored: the first base lies at the repeat boundary */
    int *depth;                  /* one per base of seq */
} pfl_consensus_result;

/* The consensus of every cluster, label[k] being flank k's label.  *out is zeroed first, filled on success (free it with
 * pfl_consensus_free) and left zeroed on failure.  rounds < 1 and the ranges of pfl_place -> PWR_ERR_RANGE; min_depth < 1
 * and the arguments of pfl_place -> PWR_ERR_ARG; PWR_ERR_INPUT as there.  Between rounds only the new backbones go up. */
int pfl_consensus(pfl_ctx *ctx, int n, const char *bases, const long long *off, const int *piece, const int *mode, const int *label,
                  int block, int extent, int max_permille, int min_depth, int rounds, pfl_consensus_result *out);
void pfl_consensus_free(pfl_consensus_result *r);
/* What pfl_consensus ends with, host only: the clusters' sequences seq[j][0 .. len[j]) and depths packed into *out (zeroed
 * first; freed and left zeroed on failure).  A negative count or length, or a null where something is to be read -> PWR_ERR_ARG. */
int pfl_consensus_pack(int nclusters, const int *label, const int *members, const int *backbone, const char *const *seq,
                       const int *const *depth, const int *len, pfl_consensus_result *out);

/* The call above on the votes of one backbone's npos positions, host only: sym[i] 0 .. 4 (4: gap), ins[i] 0 or 1 + base,
 * voters[i].  seq and depth have room for 2 * npos entries; returns the number of bases emitted. */
int pfl_call(int npos, const unsigned char *sym, const unsigned char *ins, const int *voters, int min_depth, char *seq, int *depth);

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
/* One record per cluster of r in template orientation, upper case, the sequence on one line: side "left" (the anchored
 * consensus reversed, not complemented: it ends at the boundary) or "right" (as it is), headed
 * ">left_<label> flanks=<members> bases=<n>". */
int pfl_write_flank_fasta(const char *path, const char *side, const pfl_consensus_result *r);
/* pfl_run_files, and with extent != 0 also pfl_consensus of every side's clusters (the flanks labelled by their rows'
 * labels, max_permille as for the labels) to left_fasta and right_fasta through pfl_write_flank_fasta.  extent == 0 is
 * pfl_run_files, and the four consensus parameters and the two paths are not looked at. */
int pfl_run_files_consensus(const char *seq_path, const char *info_path, const char *class_path, const char *strand_path,
                            int max_permille, int reach, int min_len, int min_size, const char *left_path, const char *right_path,
                            int extent, int block, int min_depth, int rounds, const char *left_fasta, const char *right_fasta,
                            int device, FILE *log);

#ifdef __cplusplus
}
#endif
#endif /* PFL_H */
