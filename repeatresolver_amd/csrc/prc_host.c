/* prc_host.c -- host side of the ReadCutter drop-in, plain C (the reference's host code is C).
 *
 * Reader, last-row scan, cut selection, writer, stdout lines and exit codes follow ReadCutter.c ("RC:"); the edit-distance
 * rows themselves (Occurrence, RC:491-520) go through prc_occurrences / prc_cut into the HIP kernel.
 */
#define _POSIX_C_SOURCE 200809L
#include "prc.h"

#include <stdlib.h>
#include <string.h>

static char base_of(char c)
{
    switch (c) {                                                                  /* RC:107-111, RC:176-180 */
    case 'A': case 'a': return 'a';
    case 'C': case 'c': return 'c';
    case 'G': case 'g': return 'g';
    case 'T': case 't': return 't';
    default: return 0;                                                            /* everything else is skipped */
    }
}

/* the whole file in one buffer; *n bytes */
static int slurp(const char *path, char **buf, size_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) return PWR_ERR_INPUT;
    size_t cap = (size_t)1 << 20, used = 0;
    char *b = malloc(cap);
    if (!b) { fclose(f); return PWR_ERR_NOMEM; }
    for (;;) {
        if (used == cap) { char *nb = realloc(b, cap *= 2); if (!nb) { free(b); fclose(f); return PWR_ERR_NOMEM; } b = nb; }
        const size_t got = fread(b + used, 1, cap - used, f);
        used += got;
        if (got == 0) break;
    }
    const int err = ferror(f);
    fclose(f);
    if (err) { free(b); return PWR_ERR_IO; }
    *buf = b; *n = used;
    return PWR_OK;
}

int prc_read_template(const char *path, char **templ, int *len)
{
    char *buf; size_t n;
    const int rc = slurp(path, &buf, &n);
    if (rc) return rc;
    char *t = malloc(n + 1);
    if (!t) { free(buf); return PWR_ERR_NOMEM; }
    size_t k = 0;
    for (size_t i = 0; i < n;) {                                                  /* RC:169-185: lines not starting with '>' */
        size_t e = i;
        while (e < n && buf[e] != '\n') e++;
        if (buf[i] != '>')
            for (size_t x = i; x < e; x++) { const char c = base_of(buf[x]); if (c) t[k++] = c; }
        i = e + 1;
    }
    free(buf);
    if (k > 0x7fffffff) { free(t); return PWR_ERR_RANGE; }
    *templ = t; *len = (int)k;
    return PWR_OK;
}

int prc_read_fasta(const char *path, int *nrec, char **bases, long long **off, char **last_bases, int *last_len)
{
    char *buf; size_t n;
    int rc = slurp(path, &buf, &n);
    if (rc) return rc;
    long long nh = 0;
    for (size_t i = 0; i < n;) {                                                  /* ReadCounter, RC:866-869 */
        if (buf[i] == '>') nh++;
        while (i < n && buf[i] != '\n') i++;
        i++;
    }
    if (nh > 0x7ffffffe) { free(buf); return PWR_ERR_RANGE; }
    char *b = malloc(n + 1);
    long long *o = malloc(sizeof(long long) * (size_t)(nh + 1));
    if (!b || !o) { free(buf); free(b); free(o); return PWR_ERR_NOMEM; }
    long long k = 0, r = 0;
    o[0] = 0;
    for (size_t i = 0; i < n;) {
        size_t e = i;
        while (e < n && buf[e] != '\n') e++;
        if (buf[i] == '>') { if (r > 0) o[r] = k; r++; }                          /* a record starts (RC:91-100) */
        else for (size_t x = i; x < e; x++) { const char c = base_of(buf[x]); if (c) b[k++] = c; }   /* RC:101-117; lines before
                                                                                     the first '>' join record 0 */
        i = e + 1;
    }
    free(buf);
    if (nh == 0) k = 0;
    o[nh] = k;
    /* RC:86-89: the last record meets EOF before a second '>': readcount and readlength stay those of the record before it,
     * Read holds the last record's bases over the previous one's */
    const long long P = nh >= 2 ? o[nh - 1] - o[nh - 2] : 0, Q = nh >= 1 ? o[nh] - o[nh - 1] : 0;
    if (P > 0x7fffffff) { free(b); free(o); return PWR_ERR_RANGE; }
    char *m = malloc((size_t)P + 1);
    if (!m) { free(b); free(o); return PWR_ERR_NOMEM; }
    for (long long i = 0; i < P; i++) m[i] = i < Q ? b[o[nh - 1] + i] : b[o[nh - 2] + i];
    *nrec = (int)nh; *bases = b; *off = o; *last_bases = m; *last_len = (int)P;
    return PWR_OK;
}

/* RC:525-567, literally */
int prc_scan_dense(const int *score, int len2, int len1, int cutoff, int *pos)
{
    int on = 0, lastmin = 100000, mn = 100000, ey = 0, np = 0;
    for (int i = len2 - 1; i > 0; i--) {                                          /* column 0 is never looked at */
        if (score[i] < cutoff) on = 1;
        else {
            if (on) {
                if (np > 0 && pos[np - 1] - ey > len1 / 2) pos[np++] = ey;         /* far enough from the last: a new one */
                else if (np > 0 && pos[np - 1] - ey <= len1 / 2) { if (lastmin > mn) pos[np - 1] = ey; }   /* the same one */
                else if (np == 0) pos[np++] = ey;
            }
            on = 0;
            lastmin = mn;
            mn = 100000;
        }
        if (on && score[i] < mn) { mn = score[i]; ey = i; }
    }
    return np;                                                                    /* a run still "on" at column 1 is dropped */
}

/* The same state machine fed by runs: every off column sets lastmin = mn and then mn = 100000, so the run that is flushed
 * sees the previous run's minimum exactly when one off column separates the two, and 100000 otherwise.  A run that reaches
 * column 1 is never flushed, and neither is anything below it. */
int prc_scan_runs(const int *run, int nruns, int len1, int *pos)
{
    int np = 0, have_prev = 0, prev_lo = 0, prev_mn = 0;
    for (int r = nruns - 1; r >= 0; r--) {
        const int lo = run[4 * r], hi = run[4 * r + 1], mn = run[4 * r + 2], ey = run[4 * r + 3];
        if (lo <= 1) break;
        const int lastmin = (have_prev && prev_lo - hi == 2) ? prev_mn : 100000;
        if (np > 0 && pos[np - 1] - ey > len1 / 2) pos[np++] = ey;
        else if (np > 0) { if (lastmin > mn) pos[np - 1] = ey; }
        else pos[np++] = ey;
        have_prev = 1; prev_lo = lo; prev_mn = mn;
    }
    return np;
}

static int cmp_int(const void *a, const void *b)
{
    const int x = *(const int *)a, y = *(const int *)b;
    return (x > y) - (x < y);
}

/* ascending copy of p[0 .. n) (RC:615-630 sorts all entries ascending; within one part index that is this order) */
static int *ascending(const int *p, int n)
{
    int *s = malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
    if (!s) return NULL;
    if (n) memcpy(s, p, sizeof(int) * (size_t)n);
    qsort(s, (size_t)n, sizeof(int), cmp_int);
    return s;
}

int prc_select_cuts(int parts, int len, int templ_len, int readlen, const int *pos0, int n0, const int *posL, int nL, int *cuts)
{
    const int T = templ_len;
    int *s0 = ascending(pos0, n0), *sL = parts > 1 ? ascending(posL, nL) : NULL;
    if (!s0 || (parts > 1 && !sL)) { free(s0); free(sL); return PWR_ERR_NOMEM; }
    int nc = 0;
    if (parts == 1) {                                                             /* RC:659-667 */
        for (int i = 0; i < n0; i++)
            if (s0[i] > len && readlen - s0[i] > len) cuts[nc++] = s0[i];
        free(s0);
        return nc;
    }
    /* RC:684-716: candidates by part index, in this group order; the part indices 1 .. parts-2 hold piece 0's positions
     * (RC:600-610 re-adds the last Occurrence's Positions, and that was piece 0's) */
    const int group_idx[4] = {parts - 1, 0, parts - 2, 1}, shift[4] = {0, -len, len, -2 * len};
    int j = 0;
    for (int g = 0; g < 4; g++) {
        const int idx = group_idx[g];
        const int *s = idx == parts - 1 ? sL : s0;
        const int ns = idx == parts - 1 ? nL : n0;
        for (int i = 0; i < ns; i++) {
            const int v = s[i] + shift[g];
            if (v > len && readlen - v > len) cuts[j++] = v;
        }
    }
    free(s0); free(sL);
    /* RC:719-742, in place as the reference does it: each pick overwrites the candidate at its own slot */
    for (int i = 0; i < j; i++)
        if (cuts[i] < T + T / 2) { cuts[0] = cuts[i]; nc = 1; break; }
    if (nc == 0) return 0;                                                        /* (RC reads CuttingPoints[-1] next when j > 0:
                                                                                     undefined; no candidate can follow) */
    for (int k = 0; k < 60; k++) {
        int found = 0;
        for (int i = 0; i < j; i++) {
            const int last = cuts[nc - 1];
            if (last + T / 2 < cuts[i] && cuts[i] < last + T + T / 2) { cuts[nc++] = cuts[i]; found = 1; break; }
        }
        if (!found) break;                                                        /* the state is unchanged: none would follow */
    }
    return nc;
}

/* A cut of rc(read) at c is a cut of read at readlen - c */
int prc_merge_cuts(int readlen, int nf, const int *fwd, int nr, const int *rev, int *out)
{
    if (nf < 0 || nr < 0 || (nf && !fwd) || (nr && !rev) || ((nf || nr) && !out)) return PWR_ERR_ARG;
    int n = 0;
    for (int i = 0; i < nf; i++) out[n++] = fwd[i];
    for (int i = 0; i < nr; i++) out[n++] = readlen - rev[i];
    qsort(out, (size_t)n, sizeof(int), cmp_int);
    int m = 0;
    for (int i = 0; i < n; i++)
        if (m == 0 || out[i] != out[m - 1]) out[m++] = out[i];
    return m;
}

void prc_free(void *p)
{
    free(p);
}

int prc_write_seq(const char *path, int nrec, const char *bases, const long long *off, const int *ncut, const int *cuts)
{
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;
    static char vb[1 << 20];
    setvbuf(f, vb, _IOFBF, sizeof vb);
    long long c0 = 0;
    for (int r = 0; r < nrec; r++) {
        const char *rd = bases + off[r];
        const long long L = off[r + 1] - off[r];
        const int *cp = cuts + c0;
        c0 += ncut[r];
        fputs(">\n", f);
        /* RC:898-911: "\n>\n" before base i when i == CuttingPoints[j], j < Cutting_Number; a cut point at or behind the
         * last one fired, or past the read, never fires, and neither does any after it */
        long long p = 0, prev = -1;
        for (int j = 0; j < ncut[r]; j++) {
            const long long c = cp[j];
            if (c <= prev || c >= L) break;
            fwrite(rd + p, 1, (size_t)(c - p), f);
            fputs("\n>\n", f);
            p = c; prev = c;
        }
        fwrite(rd + p, 1, (size_t)(L - p), f);
        fputc('\n', f);
    }
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

int prc_write_info(const char *path, int nrec, const int *ncut)
{
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;
    int seq = 0;
    for (int r = 0; r < nrec; r++) {
        for (int j = 0; j < ncut[r] + 1; j++) fprintf(f, "%d ", seq++);
        fputc('\n', f);
    }
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

int prc_run_files(const char *templ_path, const char *reads_path, const char *seq_path, const char *info_path, int parts,
                  int overlap, double error_cutoff, int wiggleroom, int device, FILE *log)
{
    return prc_run_files_strands(templ_path, reads_path, seq_path, info_path, parts, overlap, error_cutoff, wiggleroom, 0, device, log);
}

int prc_run_files_strands(const char *templ_path, const char *reads_path, const char *seq_path, const char *info_path, int parts,
                          int overlap, double error_cutoff, int wiggleroom, int both_strands, int device, FILE *log)
{
    fprintf(log, "parts %d, overlap %d, wiggleroom %d, error_cutoff %f\n", parts, overlap, wiggleroom, error_cutoff);   /* RC:1034 */
    char *bases = NULL, *last = NULL, *templ = NULL, *out = NULL;
    long long *off = NULL, *ooff = NULL;
    int *ncut = NULL, *cuts = NULL, *nseq = NULL, *ninfo = NULL, *scuts = NULL, *nside = NULL;
    int n = 0, P = 0, T = 0, rc = PWR_OK, ret = 1;
    prc_ctx *ctx = NULL;
    if (prc_read_fasta(reads_path, &n, &bases, &off, &last, &P)) { fprintf(log, "No Reads.\n"); fflush(log); return 1; }   /* RC:865 */
    fprintf(log, "read count %d\n", n);                                                                       /* RC:1041 */
    fflush(log);
    if (prc_read_template(templ_path, &templ, &T)) { fprintf(log, "No template.\n"); fflush(log); goto done; }  /* RC:164 */
    fprintf(log, "template length %d\n", T);                                                                  /* RC:1048 */
    if (parts < 1 || T / parts + overlap < 0) { fprintf(log, "ReadCutter: -p must be at least 1 and -l at least -%d\n", parts > 0 ? T / parts : 0); goto done; }
    /* the records as the reference writes them: 0 .. n-2 as read, then the buffer it analyses for the last one (n >= 2),
     * or one empty record (n == 1) */
    const int nout = n;
    const long long head = n >= 2 ? off[n - 1] : 0;
    out = malloc((size_t)(head + P) + 1);
    ooff = malloc(sizeof(long long) * (size_t)(nout + 1));
    nseq = calloc((size_t)nout + 1, sizeof(int));
    ninfo = calloc((size_t)nout + 1, sizeof(int));
    if (!out || !ooff || !nseq || !ninfo) { rc = PWR_ERR_NOMEM; goto fail; }
    if (head) memcpy(out, bases, (size_t)head);
    if (P) memcpy(out + head, last, (size_t)P);
    for (int i = 0; i < nout; i++) ooff[i] = i < n - 1 ? off[i] : head;
    ooff[nout] = head + P;
    free(bases); bases = NULL;
    long long ncuts_total = 0;
    if (n >= 2) {
        /* FullAnalysis of every record as written (record n-2's own analysis is overwritten by the last one's, RC:659) */
        ncut = malloc(sizeof(int) * (size_t)nout);
        if (both_strands) nside = malloc(sizeof(int) * 2 * (size_t)nout);
        rc = (ncut && (!both_strands || nside)) ? prc_create(&ctx, templ, T, device) : PWR_ERR_NOMEM;
        if (rc == PWR_OK && !both_strands) rc = prc_cut(ctx, nout, out, ooff, parts, overlap, error_cutoff, ncut, &cuts);
        if (rc == PWR_OK && both_strands)
            rc = prc_cut_strands(ctx, nout, out, ooff, parts, overlap, error_cutoff, ncut, &cuts, nside, nside + nout);
        if (rc != PWR_OK) goto fail;
        for (int i = 0; i < nout; i++) {
            const int c = i < n - 2 ? ncut[i] : ncut[n - 1];
            nseq[i] = c;
            ninfo[i] = i < n - 1 ? c : 0;                                          /* Cutting_Number[n-1] is never set */
            ncuts_total += c;
        }
        scuts = malloc(sizeof(int) * (size_t)(ncuts_total + 1));
        if (!scuts) { rc = PWR_ERR_NOMEM; goto fail; }
        long long src = 0, dst = 0, last_src = 0;
        for (int i = 0; i < nout; i++) { if (i == n - 1) last_src = src; src += ncut[i]; }
        src = 0;
        for (int i = 0; i < nout; i++) {
            const int *from = i < n - 2 ? cuts + src : cuts + last_src;
            memcpy(scuts + dst, from, sizeof(int) * (size_t)nseq[i]);
            dst += nseq[i];
            src += ncut[i];
        }
    }
    int prozent = 5;                                                                                          /* RC:1052-1079 */
    for (int i = 0; i < n; i++)
        if ((long long)i * 100 / n > prozent) { fprintf(log, "%d %% done.\n", prozent); prozent += 5; }
    fprintf(log, "Outputting results.\n");                                                                    /* RC:1082 */
    rc = prc_write_seq(seq_path, nout, out, ooff, nseq, scuts ? scuts : nseq);
    if (rc == PWR_OK) rc = prc_write_info(info_path, nout, ninfo);
fail:
    if (rc != PWR_OK) fprintf(log, "ReadCutter: %s\n", pwr_strerror(rc));
    else ret = 0;
done:
    prc_destroy(ctx);
    free(bases); free(off); free(last); free(templ); free(out); free(ooff);
    free(ncut); prc_free(cuts); free(nseq); free(ninfo); free(scuts); free(nside);
    fflush(log);
    return ret;
}
