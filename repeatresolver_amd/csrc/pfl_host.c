/* pfl_host.c -- host side of the flank labellings (include/pfl.h), plain C: which piece is a row's flank, the single-linkage
 * clustering, the chain of the two with pfl_distances (the GPU part, pfl_device.hip), the files and the drop-in's run. */
#define _POSIX_C_SOURCE 200809L
#include "pfl.h"

#include <stdlib.h>
#include <string.h>

#include "pia.h"

void pfl_free(void *p) { free(p); }

int pfl_neighbours(int npieces, const int *piece_read, const char *cls, const unsigned char *strand, int *nrows, int *row_piece,
                   int *left_piece, int *left_mode, int *right_piece, int *right_mode)
{
    if (npieces < 0 || !nrows || (npieces && (!piece_read || !cls || !row_piece || !left_piece || !left_mode || !right_piece || !right_mode)))
        return PWR_ERR_ARG;
    int t = 0;
    for (int k = 0; k < npieces; k++) {
        if (cls[k] != 'r') continue;
        /* the piece before and the piece behind, where it is a unique piece of the same read (SDA:229, SDA:237) */
        const int before = (k > 0 && piece_read[k - 1] == piece_read[k] && cls[k - 1] != 'r') ? k - 1 : -1;
        const int behind = (k + 1 < npieces && piece_read[k + 1] == piece_read[k] && cls[k + 1] != 'r') ? k + 1 : -1;
        const int rev = strand && strand[k];
        row_piece[t] = k;
        left_piece[t] = rev ? behind : before;   left_mode[t] = rev ? 2 : 1;
        right_piece[t] = rev ? before : behind;  right_mode[t] = rev ? 3 : 0;
        t++;
    }
    *nrows = t;
    return PWR_OK;
}

static int root_of(int *up, int i)
{
    while (up[i] != i) { up[i] = up[up[i]]; i = up[i]; }
    return i;
}

int pfl_cluster(int n, const int *a, const int *dist, int max_permille, int min_size, int *label_out)
{
    if (n < 0 || max_permille < 0 || min_size < 1 || (n && (!a || !dist || !label_out))) return PWR_ERR_ARG;
    if (n == 0) return PWR_OK;
    int *up = malloc(sizeof(int) * (size_t)n * 3);
    if (!up) return PWR_ERR_NOMEM;
    int *size = up + n, *name = up + 2 * (size_t)n;
    for (int i = 0; i < n; i++) { up[i] = i; size[i] = 0; name[i] = -1; }
    for (int i = 0; i < n; i++) {
        if (dist[(size_t)i * n + i] < 0) continue;                                 /* short */
        for (int j = i + 1; j < n; j++) {
            const int d = dist[(size_t)i * n + j];
            if (d < 0 || dist[(size_t)j * n + j] < 0) continue;
            const long long m = a[i] < a[j] ? a[i] : a[j];
            if (1000LL * d > (long long)max_permille * m) continue;
            const int ri = root_of(up, i), rj = root_of(up, j);
            if (ri != rj) up[ri > rj ? ri : rj] = ri > rj ? rj : ri;               /* the lower index stays the root */
        }
    }
    for (int i = 0; i < n; i++) if (dist[(size_t)i * n + i] >= 0) size[root_of(up, i)]++;
    int next = 0;
    for (int i = 0; i < n; i++) {                                                  /* a root is its component's lowest index */
        label_out[i] = -1;
        if (dist[(size_t)i * n + i] < 0) continue;
        const int r = root_of(up, i);
        if (size[r] < min_size) continue;
        if (name[r] < 0) name[r] = next++;
        label_out[i] = name[r];
    }
    free(up);
    return PWR_OK;
}

/* one side: the rows whose flank piece is >= 0, their distances, their components */
static int side_labels(pfl_ctx *ctx, int nrows, const int *fpiece, const int *fmode, const char *bases, const long long *off,
                       int max_permille, int reach, int min_len, int min_size, int *label)
{
    int n = 0, rc = PWR_OK;
    for (int t = 0; t < nrows; t++) { label[t] = -1; if (fpiece[t] >= 0) n++; }
    if (n == 0) return PWR_OK;
    int *piece = malloc(sizeof(int) * (size_t)n * 5);
    int *dist = malloc(sizeof(int) * (size_t)n * (size_t)n);
    if (!piece || !dist) { free(piece); free(dist); return PWR_ERR_NOMEM; }
    int *mode = piece + n, *row = piece + 2 * (size_t)n, *len = piece + 3 * (size_t)n, *lab = piece + 4 * (size_t)n;
    n = 0;
    for (int t = 0; t < nrows; t++) if (fpiece[t] >= 0) { piece[n] = fpiece[t]; mode[n] = fmode[t]; row[n] = t; n++; }
    rc = pfl_distances(ctx, n, bases, off, piece, mode, reach, min_len, len, dist);
    if (rc == PWR_OK) {
        for (int k = 0; k < n; k++) if (len[k] > reach) len[k] = reach;            /* a_k */
        rc = pfl_cluster(n, len, dist, max_permille, min_size, lab);
    }
    if (rc == PWR_OK) for (int k = 0; k < n; k++) label[row[k]] = lab[k];
    free(piece); free(dist);
    return rc;
}

int pfl_labels(pfl_ctx *ctx, int npieces, const char *bases, const long long *off, const int *piece_read, const char *cls,
               const unsigned char *strand, int max_permille, int reach, int min_len, int min_size, int *nrows, int *left,
               int *right)
{
    if (!ctx || npieces < 0 || !nrows || (npieces && (!bases || !off || !left || !right))) return PWR_ERR_ARG;
    if (max_permille < 0 || min_size < 1) return PWR_ERR_ARG;
    int *nb = malloc(sizeof(int) * ((size_t)npieces * 5 + 1));
    if (!nb) return PWR_ERR_NOMEM;
    const size_t np = (size_t)npieces;
    int rc = pfl_neighbours(npieces, piece_read, cls, strand, nrows, nb, nb + np, nb + 2 * np, nb + 3 * np, nb + 4 * np);
    if (rc == PWR_OK) rc = side_labels(ctx, *nrows, nb + np, nb + 2 * np, bases, off, max_permille, reach, min_len, min_size, left);
    if (rc == PWR_OK) rc = side_labels(ctx, *nrows, nb + 3 * np, nb + 4 * np, bases, off, max_permille, reach, min_len, min_size, right);
    free(nb);
    return rc;
}

int pfl_call(int npos, const unsigned char *sym, const unsigned char *ins, const int *voters, int min_depth, char *seq, int *depth)
{
    int out = 0;
    for (int i = 0; i < npos && voters[i] >= min_depth; i++) {
        if (sym[i] < 4) { seq[out] = "acgt"[sym[i]]; depth[out++] = voters[i]; }   /* 4: the gap emits nothing */
        if (ins[i]) { seq[out] = "acgt"[(ins[i] - 1) & 3]; depth[out++] = voters[i]; }
    }
    return out;
}

int pfl_consensus_pack(int nclusters, const int *label, const int *members, const int *backbone, const char *const *seq,
                       const int *const *depth, const int *len, pfl_consensus_result *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (nclusters < 0 || (nclusters && (!label || !members || !backbone || !seq || !depth || !len))) return PWR_ERR_ARG;
    long long total = 0;
    for (int j = 0; j < nclusters; j++) {
        if (len[j] < 0 || (len[j] && (!seq[j] || !depth[j]))) return PWR_ERR_ARG;
        total += len[j];
    }
    const size_t k = (size_t)nclusters;
    out->label = malloc(sizeof(int) * (k + 1)); out->members = malloc(sizeof(int) * (k + 1)); out->backbone = malloc(sizeof(int) * (k + 1));
    out->off = malloc(sizeof(long long) * (k + 1)); out->seq = malloc((size_t)total + 1); out->depth = malloc(sizeof(int) * ((size_t)total + 1));
    if (!out->label || !out->members || !out->backbone || !out->off || !out->seq || !out->depth) { pfl_consensus_free(out); return PWR_ERR_NOMEM; }
    out->nclusters = nclusters;
    out->off[0] = 0;
    for (int j = 0; j < nclusters; j++) {
        out->label[j] = label[j]; out->members[j] = members[j]; out->backbone[j] = backbone[j];
        if (len[j]) {
            memcpy(out->seq + out->off[j], seq[j], (size_t)len[j]);
            memcpy(out->depth + out->off[j], depth[j], sizeof(int) * (size_t)len[j]);
        }
        out->off[j + 1] = out->off[j] + len[j];
    }
    out->seq[total] = 0;
    return PWR_OK;
}

void pfl_consensus_free(pfl_consensus_result *r)
{
    if (!r) return;
    free(r->label); free(r->members); free(r->backbone); free(r->off); free(r->seq); free(r->depth);
    memset(r, 0, sizeof *r);
}

int pfl_write_flank_fasta(const char *path, const char *side, const pfl_consensus_result *r)
{
    if (!path || !side || !r || (strcmp(side, "left") != 0 && strcmp(side, "right") != 0)) return PWR_ERR_ARG;
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;
    const int turn = side[0] == 'l';                                               /* template orientation: a left flank ends at the boundary */
    for (int j = 0; j < r->nclusters; j++) {
        const long long lo = r->off[j], n = r->off[j + 1] - lo;
        fprintf(f, ">%s_%d flanks=%d bases=%lld\n", side, r->label[j], r->members[j], n);
        for (long long x = 0; x < n; x++) fputc(r->seq[lo + (turn ? n - 1 - x : x)] - 32, f);
        fputc('\n', f);
    }
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

int pfl_read_info(const char *path, int *npieces, int **piece_read)
{
    if (!path || !npieces || !piece_read) return PWR_ERR_ARG;
    FILE *f = fopen(path, "r");
    if (!f) return PWR_ERR_INPUT;
    int cap = 1024, n = 0, read = 0, rc = PWR_OK, ch, in_number = 0;
    long long value = 0;
    int *out = malloc(sizeof(int) * (size_t)cap);
    if (!out) { fclose(f); return PWR_ERR_NOMEM; }
    while (rc == PWR_OK) {
        ch = fgetc(f);
        if (ch >= '0' && ch <= '9') { value = in_number ? value * 10 + (ch - '0') : ch - '0'; in_number = 1; if (value > 0x7fffffff) rc = PWR_ERR_INPUT; continue; }
        if (in_number) {                                                           /* a number ends: piece `value` of read `read` */
            if (value != n) { rc = PWR_ERR_INPUT; break; }
            if (n == cap) { cap *= 2; int *no = realloc(out, sizeof(int) * (size_t)cap); if (!no) { rc = PWR_ERR_NOMEM; break; } out = no; }
            out[n++] = read;
            in_number = 0;
        }
        if (ch == EOF) break;
        if (ch == '\n') read++;
        else if (ch != ' ' && ch != '\r' && ch != '\t') rc = PWR_ERR_INPUT;
    }
    fclose(f);
    if (rc != PWR_OK) { free(out); return rc; }
    *npieces = n; *piece_read = out;
    return PWR_OK;
}

int pfl_write_labels(const char *path, int n, const int *labels)
{
    if (!path || n < 0 || (n && !labels)) return PWR_ERR_ARG;
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;
    for (int t = 0; t < n; t++) fprintf(f, "%d\n", labels[t]);
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

/* the first character of each of n lines: SeqClass letters, or the strand file's + and - as 0 and 1 */
static int read_letters(const char *path, int n, int strands, char *out)
{
    FILE *f = fopen(path, "r");
    char line[64];
    int k = 0;
    if (!f) return PWR_ERR_INPUT;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '\n') continue;
        if (k == n || (strands && line[0] != '+' && line[0] != '-')) { fclose(f); return PWR_ERR_INPUT; }
        out[k++] = strands ? (char)(line[0] == '-') : line[0];
    }
    fclose(f);
    return k == n ? PWR_OK : PWR_ERR_INPUT;
}

/* one side's consensus after the labels: the rows that have a flank there, labelled by their row's label, to path */
static int side_consensus(pfl_ctx *ctx, int npieces, int nrows, const int *fpiece, const int *fmode, const int *label, const char *bases,
                          const long long *off, int block, int extent, int max_permille, int min_depth, int rounds, const char *side,
                          const char *path, FILE *log)
{
    int n = 0;
    int *piece = malloc(sizeof(int) * ((size_t)npieces * 3 + 1));
    if (!piece) return PWR_ERR_NOMEM;
    int *mode = piece + npieces, *lab = piece + 2 * (size_t)npieces;
    for (int t = 0; t < nrows; t++) if (fpiece[t] >= 0) { piece[n] = fpiece[t]; mode[n] = fmode[t]; lab[n] = label[t]; n++; }
    pfl_consensus_result res;
    int rc = pfl_consensus(ctx, n, bases, off, piece, mode, lab, block, extent, max_permille, min_depth, rounds, &res);
    free(piece);
    if (rc != PWR_OK) return rc;
    rc = pfl_write_flank_fasta(path, side, &res);
    if (rc == PWR_OK) fprintf(log, "%s: %d consensus sequences, %lld bases\n", side, res.nclusters, res.nclusters ? res.off[res.nclusters] : 0LL);
    pfl_consensus_free(&res);
    return rc;
}

int pfl_run_files(const char *seq_path, const char *info_path, const char *class_path, const char *strand_path, int max_permille,
                  int reach, int min_len, int min_size, const char *left_path, const char *right_path, int device, FILE *log)
{
    return pfl_run_files_consensus(seq_path, info_path, class_path, strand_path, max_permille, reach, min_len, min_size, left_path,
                                   right_path, 0, 0, 0, 0, NULL, NULL, device, log);
}

int pfl_run_files_consensus(const char *seq_path, const char *info_path, const char *class_path, const char *strand_path,
                            int max_permille, int reach, int min_len, int min_size, const char *left_path, const char *right_path,
                            int extent, int block, int min_depth, int rounds, const char *left_fasta, const char *right_fasta,
                            int device, FILE *log)
{
    if (!seq_path || !info_path || !class_path || !left_path || !right_path || !log) return 1;
    if (extent && (!left_fasta || !right_fasta)) return 1;
    int n = 0, ninfo = 0, nrows = 0, rc;
    char *bases = NULL, *cls = NULL, *strand = NULL;
    long long *off = NULL;
    int *piece_read = NULL, *left = NULL, *right = NULL;
    pfl_ctx *ctx = NULL;
    unsigned long long cells = 0;
    double ms = 0.0;
    rc = pia_read_fasta(seq_path, &n, &bases, &off);
    if (rc == PWR_OK) rc = pfl_read_info(info_path, &ninfo, &piece_read);
    if (rc == PWR_OK && ninfo > n) {
        fprintf(log, "FlankClusterer: %s holds %d pieces, %s lists %d.\n", seq_path, n, info_path, ninfo);
        rc = PWR_ERR_INPUT;
    }
    if (rc == PWR_OK && ninfo < n) {                                               /* the last record's own pieces (pfl.h) */
        const int last_read = ninfo ? piece_read[ninfo - 1] : 0;
        int *more = realloc(piece_read, sizeof(int) * (size_t)n);
        if (!more) rc = PWR_ERR_NOMEM;
        else {
            piece_read = more;
            fprintf(log, "%s lists %d of %d pieces: the last read takes the other %d.\n", info_path, ninfo, n, n - ninfo);
            for (int k = ninfo; k < n; k++) piece_read[k] = last_read;
        }
    }
    if (rc == PWR_OK) {
        fprintf(log, "pieces %d\n", n);
        cls = malloc((size_t)n + 1); left = malloc(sizeof(int) * ((size_t)n + 1)); right = malloc(sizeof(int) * ((size_t)n + 1));
        if (strand_path) strand = malloc((size_t)n + 1);
        if (!cls || !left || !right || (strand_path && !strand)) rc = PWR_ERR_NOMEM;
    }
    if (rc == PWR_OK) rc = read_letters(class_path, n, 0, cls);
    if (rc == PWR_OK && strand_path) rc = read_letters(strand_path, n, 1, strand);
    if (rc == PWR_OK) rc = pfl_create(&ctx, device);
    if (rc == PWR_OK) rc = pfl_labels(ctx, n, bases, off, piece_read, cls, (const unsigned char *)strand, max_permille, reach, min_len,
                                      min_size, &nrows, left, right);
    if (rc == PWR_OK) rc = pfl_write_labels(left_path, nrows, left);
    if (rc == PWR_OK) rc = pfl_write_labels(right_path, nrows, right);
    if (rc == PWR_OK && extent) {                                                  /* the sequence of every cluster, side by side */
        int *nb = malloc(sizeof(int) * ((size_t)n * 5 + 1)), rows = 0;
        const size_t np = (size_t)n;
        if (!nb) rc = PWR_ERR_NOMEM;
        if (rc == PWR_OK) rc = pfl_neighbours(n, piece_read, cls, (const unsigned char *)strand, &rows, nb, nb + np, nb + 2 * np, nb + 3 * np, nb + 4 * np);
        if (rc == PWR_OK) rc = side_consensus(ctx, n, rows, nb + np, nb + 2 * np, left, bases, off, block, extent, max_permille, min_depth,
                                              rounds, "left", left_fasta, log);
        if (rc == PWR_OK) rc = side_consensus(ctx, n, rows, nb + 3 * np, nb + 4 * np, right, bases, off, block, extent, max_permille,
                                              min_depth, rounds, "right", right_fasta, log);
        free(nb);
    }
    if (rc == PWR_OK) {
        int kl = 0, kr = 0, hl = 0, hr = 0;
        for (int t = 0; t < nrows; t++) {
            if (left[t] >= 0) hl++;
            if (right[t] >= 0) hr++;
            if (left[t] >= kl) kl = left[t] + 1;
            if (right[t] >= kr) kr = right[t] + 1;
        }
        pfl_get_stats(ctx, &cells, &ms);
        fprintf(log, "rows %d\n", nrows);
        fprintf(log, "left: %d rows in %d clusters; right: %d rows in %d clusters\n", hl, kl, hr, kr);
        fprintf(log, "cells %llu, kernel %.3f ms\n", cells, ms);
        if (extent) fprintf(log, "Files written: %s %s %s %s\n", left_path, right_path, left_fasta, right_fasta);
        else fprintf(log, "Files written: %s %s\n", left_path, right_path);
    } else fprintf(log, "FlankClusterer: %s\n", pwr_strerror(rc));
    pfl_destroy(ctx);
    free(bases); free(off); free(piece_read); free(cls); free(strand); free(left); free(right);
    return rc == PWR_OK ? 0 : 1;
}
