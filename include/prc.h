/*
 * prc.h -- C ABI of the MI355X-native ReadCutter (part of libpwr.so), the first tool of the RepeatResolver pipeline: it cuts
 * raw reads where a repeat instance ends and writes the Seq.fasta that InitialAligner (pia.h) reads.
 *
 * Reference: PhilippBongartz/RepeatResolver, ReadCutter.c ("RC:").  Its boundary is the process
 * (`./ReadCutter template.fasta reads.fasta [-p parts] [-l overlap] [-e error_cutoff] [-w wiggleroom] [-o Seq] [-r Info]`,
 * RC:939-1112).  Inside, FullAnalysis (RC:581-757) maps the first and the last of `parts` template pieces into each read with
 * a semi-global edit distance (Occurrence, RC:491-568) and turns the hits into cut points.  The edit-distance rows run on the
 * GPU (prc_occurrences, prc_cut); the scan of the last row, the cut selection, the reader and the writer are plain C.
 * Error codes are those of pwr.h.
 */
#ifndef PRC_H
#define PRC_H

#include <stdio.h>

#include "pwr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRC_MAX_PART 40960       /* longest template piece the kernel takes (20 words of 32 bits per lane); RC:15 says 40000 */
#define PRC_RUN_CAP 8            /* runs below the cutoff kept per job in the first launch; more are re-run with room */

typedef struct prc_ctx prc_ctx;

/* The template (acgt in either case; anything else is refused with PWR_ERR_INPUT, as in pia_create) is kept by the
 * context.  Template bytes past templ_len, which a piece reaches when overlap > 0, match no base (RC:191-192 copies an
 * uninitialised byte there). */
int prc_create(prc_ctx **out, const char *templ, int templ_len, int device);
void prc_destroy(prc_ctx *ctx);

/* Occurrence (RC:491-568) of the pieces FullAnalysis queries -- piece 0 and piece parts-1, or piece 0 alone when
 * parts == 1 (RC:600) -- in each of nreads reads (bases: acgt in either case, off[nreads + 1] offsets).  Job k = read j,
 * query q (q = 0 for piece 0, 1 for piece parts-1; nq = parts > 1 ? 2 : 1, k = j * nq + q) has its positions at
 * (*pos)[pos_off[k] .. pos_off[k + 1]) in the reference's order (descending).  pos_off holds nreads * nq + 1 entries;
 * *pos is malloc'ed (prc_free).  parts < 1 or steps + overlap < 0 -> PWR_ERR_ARG; a piece longer than PRC_MAX_PART ->
 * PWR_ERR_RANGE. */
int prc_occurrences(prc_ctx *ctx, int nreads, const char *bases, const long long *off, int parts, int overlap,
                    double error_cutoff, long long *pos_off, int **pos);
/* FullAnalysis (RC:581-757) of each read taken on its own: ncut[j] cut points of read j, concatenated in *cuts (malloc'ed,
 * prc_free).  (RC:1053-1079 applies it to a different buffer for the last record of a file: prc_read_fasta.) */
int prc_cut(prc_ctx *ctx, int nreads, const char *bases, const long long *off, int parts, int overlap, double error_cutoff,
            int *ncut, int **cuts);
/* Reads from either strand.  rc(r)[x] = comp(r[L-1-x]), a<->t, c<->g.  prc_occurrences of every read and of its reverse
 * complement from one copy of the bases (a job carries its strand): job k = (j * 2 + s) * nq + q is read j, strand s
 * (1: rc(read j)), query q, and its positions are in the coordinates of that orientation.  pos_off holds nreads * 2 * nq + 1
 * entries. */
int prc_occurrences_strands(prc_ctx *ctx, int nreads, const char *bases, const long long *off, int parts, int overlap,
                            double error_cutoff, long long *pos_off, int **pos);
/* With F = prc_cut(read) and R = prc_cut(rc(read)): the read's cut points are the ascending union of F and
 * {readlen - c : c in R}, each value once (prc_merge_cuts) -- cutting rc(read) at c is cutting read at readlen - c, so a
 * reverse read is cut where its mirror image would be, and a read holding copies in both orientations is cut at both.
 * nfwd[j] = |F|, nrev[j] = |R|.  No strand is decided here and nothing is turned: that is pia_align_strands' part. */
int prc_cut_strands(prc_ctx *ctx, int nreads, const char *bases, const long long *off, int parts, int overlap,
                    double error_cutoff, int *ncut, int **cuts, int *nfwd, int *nrev);
/* DP cells the reference fills for the calls so far (piece length x read length per query; the _strands entries count both
 * orientations) and the summed kernel time, ms. */
int prc_get_stats(prc_ctx *ctx, unsigned long long *cells, double *kernel_ms);
void prc_free(void *p);

/* ---- host side, plain C (prc_host.c), usable without a GPU ---- */
/* ReadingTemplate (RC:155-193): every line that does not start with '>' contributes its aAcCgGtT, lower-cased. */
int prc_read_template(const char *path, char **templ, int *len);
/* ReadCounter + ReadingFasta (RC:66-135, RC:858-872) in one pass.  Records start at lines that begin with '>' (lines before
 * the first one join record 0); only aAcCgGtT are kept, lower-cased.  *nrec records at (*bases)[(*off)[i] .. (*off)[i + 1]).
 * ReadingFasta hits EOF on the last record before a second '>' and keeps the previous record's count and length, so the
 * reference analyses and writes, for the last record, *last_len = length of the record before it (0 for a one-record file)
 * bases of the buffer (last + previous[len(last):])[:len(previous)]: *last_bases (malloc'ed, also when *last_len is 0). */
int prc_read_fasta(const char *path, int *nrec, char **bases, long long **off, char **last_bases, int *last_len);
/* The scan of the last DP row in Occurrence (RC:525-567) from the dense per-column scores score[0 .. len2): writes the
 * positions to pos (room for (len2 + 1) / 2) and returns their number. */
int prc_scan_dense(const int *score, int len2, int len1, int cutoff, int *pos);
/* The same scan from the runs of columns with score < cutoff, in ascending column order: run r = run[4r .. 4r + 4) =
 * {first column, last column, minimum score, largest column holding the minimum}.  pos needs room for nruns. */
int prc_scan_runs(const int *run, int nruns, int len1, int *pos);
/* The cut selection of FullAnalysis (RC:614-755) for one read of length readlen: pos0 / posL are the positions of piece 0 /
 * piece parts-1 in the reference's order (posL ignored when parts == 1).  Writes the cut points to cuts (room for
 * 3 * n0 + 2 * nL + 1) and returns their number. */
int prc_select_cuts(int parts, int len, int templ_len, int readlen, const int *pos0, int n0, const int *posL, int nL, int *cuts);
/* The merge of prc_cut_strands for one read: fwd[0 .. nf) cut points of the read, rev[0 .. nr) of its reverse complement; out
 * (room nf + nr) gets the ascending union of fwd and {readlen - c}, each value once.  Returns their number. */
int prc_merge_cuts(int readlen, int nf, const int *fwd, int nr, const int *rev, int *out);
/* OutputOfCuts (RC:887-913) for nrec records: ">\n", the bases with "\n>\n" before each cut point, "\n".  ncut[i] cut points
 * of record i, concatenated in cuts. */
int prc_write_seq(const char *path, int nrec, const char *bases, const long long *off, const int *ncut, const int *cuts);
/* OutputOfReadSeqInfo (RC:918-937): per record ncut[i] + 1 running sequence numbers, each followed by a space, then "\n". */
int prc_write_info(const char *path, int nrec, const int *ncut);
/* main() of the reference from the "parts ..." line on (RC:1034-1110): same files, same stdout including the progress lines;
 * returns the process exit code.  (The caller prints the two default output names first, RC:972-973.) */
int prc_run_files(const char *templ_path, const char *reads_path, const char *seq_path, const char *info_path, int parts,
                  int overlap, double error_cutoff, int wiggleroom, int device, FILE *log);
/* The same with `-b 1` of the drop-in: both_strands != 0 uses prc_cut_strands where prc_run_files uses prc_cut; everything
 * else, the last-record buffer included, stays.  The pieces are written in the read's own orientation and order. */
int prc_run_files_strands(const char *templ_path, const char *reads_path, const char *seq_path, const char *info_path, int parts,
                          int overlap, double error_cutoff, int wiggleroom, int both_strands, int device, FILE *log);

#ifdef __cplusplus
}
#endif
#endif /* PRC_H */
