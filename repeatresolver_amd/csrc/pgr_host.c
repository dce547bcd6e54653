/* pgr_host.c -- host side of RepeatResolver's group refinement, plain C: the window reader, the MaxCorrs slice and the
 * preparation in main() (RR:293-429, RR:609-646, RR:3977-4014); below them DropOff_Subdivision and the helpers of both
 * drop-off subdivisions (RR:568-585, RR:1823-1865, RR:3180-3271); at the end the reassignment chain of Kmeans (RR:2726-2755). */
#define _POSIX_C_SOURCE 200809L
#include "pgr.h"
#include "base_code.h"
#include "pgr_internal.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

void pgr_word_major(const unsigned long long *sets, int sc, const int *pick, size_t n, unsigned long long *out)
{
    for (size_t c = 0; c < n; c++) {
        const unsigned long long *set = sets + (pick ? (size_t)pick[c] : c) * sc;
        for (int w = 0; w < sc; w++) out[(size_t)w * n + c] = set[w];
    }
}

void pgr_window_free(pgr_window *win)
{
    if (!win) return;
    free(win->kept); free(win->groups); free(win->local_coverage); free(win->coverage);
    memset(win, 0, sizeof *win);
}

int pgr_read_window(int rows, int width, const unsigned char *text, int von, int bis, pgr_window *win)
{
    if (!win) return PWR_ERR_ARG;
    memset(win, 0, sizeof *win);
    if (rows <= 0 || width <= 0 || !text) return PWR_ERR_ARG;
    if (rows > PGR_MAX_ROWS || width > PGR_MAX_COLUMNS - 3) return PWR_ERR_RANGE;  /* RR:291, RR:322 */
    if (von == -1 && bis == -1) { von = 0; bis = PGR_MAX_COLUMNS; }                /* RR:3948-3952 */
    if (bis > width - 1) bis = width - 1;                                          /* RR:328 */
    if (von < 0 || von > bis) return PWR_ERR_ARG;
    const int w = bis + 1 - von;                                                   /* RR:374 */
    win->rows = rows; win->von = von; win->bis = bis; win->width = w;
    win->kept = malloc((size_t)rows);
    if (!win->kept) return PWR_ERR_NOMEM;
    int kept = 0;
    for (int r = 0; r < rows; r++) {
        const unsigned char *line = text + (size_t)r * width;
        win->kept[r] = line[von] != ' ' && line[bis] != ' ';                       /* RR:330 */
        kept += win->kept[r];
    }
    const int sc = kept / 64 + 1;                                                  /* RR:375 */
    win->kept_rows = kept; win->sc = sc;
    win->groups = calloc((size_t)w * 5 * sc, 8);
    win->local_coverage = calloc((size_t)w * sc, 8);
    win->coverage = calloc((size_t)w, sizeof(int));
    if (!win->groups || !win->local_coverage || !win->coverage) { pgr_window_free(win); return PWR_ERR_NOMEM; }
    int j = 0;
    for (int r = 0; r < rows; r++) {
        if (!win->kept[r]) continue;
        const unsigned char *line = text + (size_t)r * width + von;
        const unsigned long long bit = 1ull << (j % 64);
        for (int i = 0; i < w; i++) {
            const int k = base_code(line[i]);                                  /* RR:336-359 */
            if (k < 5) {                                                           /* RR:402-420 */
                win->groups[((size_t)i * 5 + k) * sc + j / 64] |= bit;
                win->local_coverage[(size_t)i * sc + j / 64] |= bit;
                win->coverage[i]++;
            }
        }
        j++;
    }
    return PWR_OK;
}

int pgr_slice_maxcorrs(const double *full, int nfull, int von, int bis, double *out)
{
    if (!full || !out || von < 0 || bis < von) return PWR_ERR_ARG;
    if ((long long)(bis + 1) * 5 > nfull) return PWR_ERR_INPUT;                    /* the reference would leave the rest unset */
    memcpy(out, full + (size_t)von * 5, sizeof(double) * (size_t)(bis + 1 - von) * 5);   /* i / 5 in [von, bis], RR:631 */
    return PWR_OK;
}

int pgr_read_maxcorrs_file(const char *path, int von, int bis, double **out, int *n)
{
    if (!path || !out || !n || von < 0 || bis < von) return PWR_ERR_ARG;
    FILE *f = fopen(path, "r");
    if (!f) return PWR_ERR_INPUT;                                                  /* RR:621 */
    const size_t want = (size_t)(bis + 1 - von) * 5;
    double *mc = calloc(want ? want : 1, sizeof(double));
    if (!mc) { fclose(f); return PWR_ERR_NOMEM; }
    char buffer[101];
    long long i = 0;
    size_t j = 0;
    while (fgets(buffer, 100, f)) {                                                /* RR:629 */
        if (i / 5 >= von && i / 5 <= bis && j < want) {
            sscanf(buffer, "%lf", mc + j);                                         /* RR:633 */
            j++;
        }
        i++;
    }
    fclose(f);
    *out = mc; *n = (int)j;
    return PWR_OK;
}

double pgr_default_cutoff(double cutoff, int width)
{
    if (cutoff < 0.1) cutoff = -1.0 * log10(1.0 / (double)(width * 5.0));          /* RR:3977 */
    return cutoff;
}

int pgr_restrict_coverage(int width, const int *coverage, double *maxcorrs, int *maxcov)
{
    if (width <= 0 || !coverage || !maxcorrs) return PWR_ERR_ARG;
    int m = 0;
    for (int i = 0; i < width; i++) if (coverage[i] > m) m = coverage[i];           /* RR:4004-4008 */
    for (size_t i = 0; i < (size_t)width * 5; i++)
        if (coverage[i / 5] * 10 < m * 9) maxcorrs[i] = 0.0;                       /* RR:4011-4014 */
    if (maxcov) *maxcov = m;
    return PWR_OK;
}

/* ---- the drop-off subdivisions: stage 1 and the helpers of both (RR:568-585, RR:1823-1865, RR:3180-3271) ---- */

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int pgr_compress_labels(int n, int *labels)
{
    if (n < 0 || (n > 0 && !labels)) return PWR_ERR_ARG;
    int max = 0;
    for (int i = 0; i < n; i++) if (max < labels[i]) max = labels[i];              /* RR:1829 */
    int *replace = malloc(sizeof(int) * ((size_t)max + 1));
    if (!replace) return PWR_ERR_NOMEM;
    for (int i = 0; i < max + 1; i++) replace[i] = -1;
    max = 0;
    for (int i = 0; i < n; i++) {
        if (labels[i] > -1) {                                                      /* RR:1835-1838 */
            if (replace[labels[i]] < 0) { replace[labels[i]] = max; max++; }
            labels[i] = replace[labels[i]];
        }
    }
    free(replace);
    return max;
}

int pgr_complete_labels(int rows, const unsigned char *kept, const int *labels, int *out)
{
    if (rows < 0 || !kept || !out) return PWR_ERR_ARG;
    int j = 0;
    for (int i = 0; i < rows; i++) {                                               /* RR:1852-1863 */
        if (kept[i]) {
            if (!labels) return PWR_ERR_ARG;
            out[i] = labels[j];
            j++;
        } else {
            out[i] = -1;
        }
    }
    return PWR_OK;
}

int pgr_write_subdivision(const char *path, const int *labels, int rows)
{
    if (!path || rows < 0 || (rows > 0 && !labels)) return PWR_ERR_ARG;
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;                                                     /* RR:573-577 */
    for (int i = 0; i < rows; i++) {                                               /* RR:579-583 */
        if (i != 0) fprintf(f, "\n");
        fprintf(f, "%d", labels[i]);
    }
    if (fclose(f) != 0) return PWR_ERR_IO;
    return PWR_OK;
}

int pgr_subdivision_name(char *buf, size_t n, const char *stage, int von, int bis, const char *msa)
{
    if (!buf || !stage || !msa) return PWR_ERR_ARG;
    if (von == -1 && bis == -1) { von = 0; bis = PGR_MAX_COLUMNS; }                /* RR:3948-3952 */
    const int len = snprintf(buf, n, "%sSubdivisionOf_%d_%d_%s", stage, von, bis, msa);   /* RR:4041-4046 */
    if (len < 0 || (size_t)len >= n) return PWR_ERR_RANGE;
    return PWR_OK;
}

int pgr_dropoff_subdivision(const pgr_result *r, int mingroup, int *labels, int *parts, double *ms2)
{
    if (!r || !parts || mingroup < 0 || r->kept_rows < 0 || r->nsig < 0 || (r->kept_rows > 0 && !labels)) return PWR_ERR_ARG;
    if (r->nsig > 0 && (!r->significant || !r->maxcorrs || !r->sizes || !r->drop_off || !r->c_groups)) return PWR_ERR_ARG;
    if (r->sc != r->kept_rows / 64 + 1) return PWR_ERR_ARG;
    const double t0 = now_ms();
    const int signumber = r->kept_rows, sc = r->sc;
    const double dropoffcutoff = 0.0001;                                           /* RR:4036 */
    int anzahl = 0;
    int *I = malloc(sizeof(int) * ((size_t)r->nsig + 1));
    if (!I) return PWR_ERR_NOMEM;
    for (int s = 0; s < r->nsig; s++) {                                            /* RR:3186-3193, sizecutoff = -1 */
        if (r->significant[s] < 0 || r->significant[s] >= r->width * 5) { free(I); return PWR_ERR_ARG; }
        if (r->maxcorrs[r->significant[s]] > r->cutoff && r->sizes[s] > -1) { I[anzahl] = s; anzahl++; }
    }
    const double *Drop_Off = r->drop_off;
    const int *Sizes = r->sizes;
#define MAXCORRS(s) (r->maxcorrs[r->significant[s]])
    int i, j, k;
    for (i = 0; i < anzahl; i++) {                                                 /* RR:3199-3213, swap for swap */
        for (j = i + 1; j < anzahl; j++) {
            if (Drop_Off[I[i]] > Drop_Off[I[j]]) { k = I[i]; I[i] = I[j]; I[j] = k; }
            else if (Drop_Off[I[i]] == Drop_Off[I[j]]) {
                if (Sizes[I[i]] < Sizes[I[j]]) { k = I[i]; I[i] = I[j]; I[j] = k; }
                else if (Sizes[I[i]] == Sizes[I[j]]) {
                    if (MAXCORRS(I[i]) < MAXCORRS(I[j])) { k = I[i]; I[i] = I[j]; I[j] = k; }
                }
            }
        }
    }
#undef MAXCORRS
    const double t1 = now_ms();
    for (i = 0; i < signumber; i++) labels[i] = 0;                                 /* RR:3221 */
    int number = 1, number2 = 1, drinne, draus;
    for (i = 0; i < anzahl; i++) {                                                 /* RR:3225-3263 */
        if (Drop_Off[I[i]] < dropoffcutoff) {
            const unsigned long long *cg = r->c_groups + (size_t)I[i] * sc;
            for (k = 0; k < number; k++) {
                drinne = 0;
                draus = 0;
                for (j = 0; j < signumber; j++) {
                    if (labels[j] == k) {
                        if ((cg[j / 64] >> (j % 64)) & 1ull) drinne += 1;
                        else draus += 1;
                    }
                }
                if (drinne > mingroup && draus > mingroup) {
                    for (j = 0; j < signumber; j++) {
                        if (labels[j] == k) {
                            if ((cg[j / 64] >> (j % 64)) & 1ull) labels[j] = number2;
                            else labels[j] = number2 + 1;
                        }
                    }
                    number2 += 2;
                }
            }
            number = pgr_compress_labels(signumber, labels);                       /* RR:3259-3260 */
            if (number < 0) { free(I); return number; }
        }
    }
    free(I);
    *parts = number;
    if (ms2) { ms2[0] = t1 - t0; ms2[1] = now_ms() - t1; }
    return PWR_OK;
}

/* ---- the k-means subdivision: the sequential chain (RR:2726-2755) ---- */

int pgr_kmeans_reassign(int anzahl, const unsigned short *scores, int mingroup, int *clusternumber)
{
    if (anzahl < 0 || (anzahl > 0 && (!scores || !clusternumber))) return PWR_ERR_ARG;
    int *Clustersize = calloc((size_t)anzahl + 1, sizeof(int));
    if (!Clustersize) return PWR_ERR_NOMEM;
    int i, j, min;
    for (i = 0; i < anzahl; i++) {
        if (clusternumber[i] < 0 || clusternumber[i] >= anzahl) { free(Clustersize); return PWR_ERR_ARG; }
        Clustersize[clusternumber[i]]++;                                           /* RR:2722 */
    }
    for (min = 2; min < mingroup; min++) {
        for (i = 0; i < anzahl; i++) {
            if (Clustersize[clusternumber[i]] <= min) {                            /* RR:2731 */
                const unsigned short *row = scores + (size_t)i * anzahl;
                int best_score = 0, best_j = 0;
                for (j = 0; j < anzahl; j++) {
                    if (Clustersize[j] >= min && clusternumber[i] != j) {          /* RR:2737 */
                        const int score = row[j];
                        if (score > best_score && i != j) { best_score = score; best_j = j; }
                    }
                }
                Clustersize[clusternumber[i]]--;                                   /* RR:2747-2749 */
                clusternumber[i] = best_j;
                Clustersize[best_j]++;
            }
        }
    }
    free(Clustersize);
    return PWR_OK;
}

/* ---- the connection of the windows (SimDataAssessment.py:359-391, "SDA:") ---- */

void pgr_connection_free(pgr_connection *c)
{
    if (!c) return;
    free(c->matrix); free(c->best); free(c->confidence); free(c->mutual);
    memset(c, 0, sizeof *c);
}

/* ProbabilityMatrix (SDA:359-370): *out is calloc'ed [*k1][*k2] */
static int probability_matrix(int rows, const int *r1, const int *r2, int k1, int k2, double **out)
{
    double *m = calloc((size_t)k1 * k2, sizeof(double));
    int *sums = calloc((size_t)k1, sizeof(int));
    if (!m || !sums) { free(m); free(sums); return PWR_ERR_NOMEM; }
    for (int t = 0; t < rows; t++) {
        if (r1[t] > -1 && r2[t] > -1) { sums[r1[t]]++; m[(size_t)r1[t] * k2 + r2[t]] += 1.0; }   /* SDA:361-364 */
    }
    for (int a = 0; a < k1; a++)
        for (int b = 0; b < k2; b++)
            if (sums[a] > 0) m[(size_t)a * k2 + b] /= (double)sums[a];                            /* SDA:365-368 */
    free(sums);
    *out = m;
    return PWR_OK;
}

/* acc[n][k] . m[k][p], the sum over k ascending */
static double *product(const double *acc, const double *m, int n, int k, int p)
{
    double *o = calloc((size_t)n * p, sizeof(double));
    if (!o) return NULL;
    for (int i = 0; i < n; i++)
        for (int l = 0; l < k; l++) {
            const double x = acc[(size_t)i * k + l];
            if (x == 0.0) continue;                                                   /* adds +0.0: no value changes */
            for (int j = 0; j < p; j++) o[(size_t)i * p + j] += x * m[(size_t)l * p + j];
        }
    return o;
}

/* the chain PM(order[0], order[1]) . PM(order[1], order[2]) ... over the labellings in the given order (SDA:376-383) */
static int chained(int nres, int rows, const int *labels, const int *K, int backward, double **out)
{
    double *acc = NULL;
    for (int s = 0; s + 1 < nres; s++) {
        const int a = backward ? nres - 1 - s : s, b = backward ? nres - 2 - s : s + 1, first = backward ? nres - 1 : 0;
        double *m = NULL;
        const int rc = probability_matrix(rows, labels + (size_t)a * rows, labels + (size_t)b * rows, K[a], K[b], &m);
        if (rc) { free(acc); return rc; }
        if (!acc) { acc = m; continue; }
        double *next = product(acc, m, K[first], K[a], K[b]);
        free(acc); free(m);
        if (!next) return PWR_ERR_NOMEM;
        acc = next;
    }
    *out = acc;
    return PWR_OK;
}

int pgr_connect(int nres, int rows, const int *labels, pgr_connection *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (nres < 2 || rows <= 0 || !labels) return PWR_ERR_ARG;
    int *K = malloc(sizeof(int) * (size_t)nres);
    if (!K) return PWR_ERR_NOMEM;
    for (int r = 0; r < nres; r++) {
        int max = -1;
        for (int t = 0; t < rows; t++) {
            const int l = labels[(size_t)r * rows + t];
            if (l < -1) { free(K); return PWR_ERR_ARG; }
            if (l > max) max = l;
        }
        if (max < 0) { free(K); return PWR_ERR_ARG; }
        K[r] = max + 1;
    }
    const int k1 = K[0], k2 = K[nres - 1];
    double *fw = NULL, *bw = NULL;
    int rc = chained(nres, rows, labels, K, 0, &fw);                                  /* [k1][k2] */
    if (!rc) rc = chained(nres, rows, labels, K, 1, &bw);                             /* [k2][k1] */
    free(K);
    out->k_first = k1; out->k_last = k2;
    out->best = malloc(sizeof(int) * (size_t)k1);
    out->confidence = malloc(sizeof(double) * (size_t)k1);
    out->mutual = malloc(sizeof(int) * (size_t)k1);
    if (!rc && (!out->best || !out->confidence || !out->mutual)) rc = PWR_ERR_NOMEM;
    if (rc) { free(fw); free(bw); pgr_connection_free(out); return rc; }
    for (int a = 0; a < k1; a++) {
        double summe = 0.0;
        for (int b = 0; b < k2; b++) { fw[(size_t)a * k2 + b] *= bw[(size_t)b * k1 + a]; summe += fw[(size_t)a * k2 + b]; }   /* SDA:384, 388 */
        if (summe > 0.0)
            for (int b = 0; b < k2; b++) fw[(size_t)a * k2 + b] /= summe;             /* SDA:389-391 */
    }
    free(bw);
    out->matrix = fw;
    for (int a = 0; a < k1; a++) {
        double maxi = 0.0;
        int maxtt = -1;
        for (int b = 0; b < k2; b++)
            if (fw[(size_t)a * k2 + b] > maxi) { maxi = fw[(size_t)a * k2 + b]; maxtt = b; }   /* SDA:399-405 */
        out->best[a] = maxtt; out->confidence[a] = maxi; out->mutual[a] = 0;
        if (maxtt < 0) continue;
        int is_max = 1;
        for (int t = 0; t < k1; t++) if (fw[(size_t)t * k2 + maxtt] > maxi) is_max = 0;
        out->mutual[a] = is_max;
    }
    return PWR_OK;
}

/* ---- the windows' labellings threaded into whole copies: the discrete counterpart of pgr_connect (no reference) ---- */

void pgr_threads_free(pgr_threads *t)
{
    if (!t) return;
    free(t->first); free(t->last); free(t->offset); free(t->thread_of); free(t->row_thread); free(t->row_conflict);
    memset(t, 0, sizeof *t);
}

/* next[a] = the label of `r2` linked with label a of `r1`, -1: none; linked[b] = 1 where label b of r2 has such a partner */
static int links(int rows, const int *r1, const int *r2, int k1, int k2, int *next, unsigned char *linked)
{
    int *C = calloc((size_t)k1 * k2, sizeof(int)), *col_best = malloc(sizeof(int) * (size_t)k2);
    if (!C || !col_best) { free(C); free(col_best); return PWR_ERR_NOMEM; }
    for (int t = 0; t < rows; t++)
        if (r1[t] > -1 && r2[t] > -1) C[(size_t)r1[t] * k2 + r2[t]]++;
    for (int b = 0; b < k2; b++) {                                                    /* the first largest of every column */
        int best = 0;
        for (int a = 1; a < k1; a++) if (C[(size_t)a * k2 + b] > C[(size_t)best * k2 + b]) best = a;
        col_best[b] = best;
        linked[b] = 0;
    }
    for (int a = 0; a < k1; a++) {
        int best = 0;                                                                 /* the first largest of the row */
        for (int b = 1; b < k2; b++) if (C[(size_t)a * k2 + b] > C[(size_t)a * k2 + best]) best = b;
        next[a] = -1;
        if (C[(size_t)a * k2 + best] > 0 && col_best[best] == a) { next[a] = best; linked[best] = 1; }
    }
    free(C); free(col_best);
    return PWR_OK;
}

int pgr_thread(int nres, int rows, const int *labels, pgr_threads *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (nres < 2 || rows <= 0 || !labels) return PWR_ERR_ARG;
    int rc = PWR_OK, *next = NULL;
    unsigned char *occurs = NULL, *linked = NULL;
    out->offset = calloc((size_t)nres + 1, sizeof(int));
    if (!out->offset) return PWR_ERR_NOMEM;
    int *off = out->offset;
    for (int i = 0; i < nres; i++) {                                                  /* as pgr_connect */
        int max = -1;
        for (int t = 0; t < rows; t++) {
            const int l = labels[(size_t)i * rows + t];
            if (l < -1) { rc = PWR_ERR_ARG; goto fail; }
            if (l > max) max = l;
        }
        if (max < 0) { rc = PWR_ERR_ARG; goto fail; }
        if (off[i] > 0x7fffffff - (max + 1)) { rc = PWR_ERR_RANGE; goto fail; }
        off[i + 1] = off[i] + max + 1;
    }
    const size_t n = (size_t)off[nres];
    out->nres = nres; out->rows = rows;
    out->thread_of = malloc(sizeof(int) * n); out->first = malloc(sizeof(int) * n); out->last = malloc(sizeof(int) * n);
    out->row_thread = malloc(sizeof(int) * (size_t)rows); out->row_conflict = malloc(sizeof(int) * (size_t)rows);
    next = malloc(sizeof(int) * n); occurs = calloc(n, 1); linked = calloc(n, 1);
    if (!out->thread_of || !out->first || !out->last || !out->row_thread || !out->row_conflict || !next || !occurs || !linked) {
        rc = PWR_ERR_NOMEM;
        goto fail;
    }
    for (int i = 0; i < nres; i++)
        for (int t = 0; t < rows; t++)
            if (labels[(size_t)i * rows + t] > -1) occurs[off[i] + labels[(size_t)i * rows + t]] = 1;
    for (int i = 0; i + 1 < nres; i++) {
        rc = links(rows, labels + (size_t)i * rows, labels + (size_t)(i + 1) * rows, off[i + 1] - off[i], off[i + 2] - off[i + 1],
                   next + off[i], linked + off[i + 1]);
        if (rc) goto fail;
    }
    for (int a = off[nres - 1]; a < off[nres]; a++) next[a] = -1;                      /* the last labelling links to nothing */
    int threads = 0;
    for (size_t e = 0; e < n; e++) out->thread_of[e] = -1;
    for (int i = 0; i < nres; i++)
        for (int a = 0; a < off[i + 1] - off[i]; a++) {
            if (!occurs[off[i] + a] || linked[off[i] + a]) continue;                  /* no label, or not the first of its thread */
            int j = i, l = a;
            for (;;) {
                out->thread_of[off[j] + l] = threads;
                if (next[off[j] + l] < 0) break;
                l = next[off[j] + l]; j++;
            }
            out->first[threads] = i; out->last[threads] = j;
            threads++;
        }
    out->nthreads = threads;
    for (int t = 0; t < rows; t++) {
        int thread = -1, conflict = 0;
        for (int i = 0; i < nres; i++) {
            const int l = labels[(size_t)i * rows + t];
            if (l < 0) continue;
            const int x = out->thread_of[off[i] + l];
            if (thread < 0) thread = x;
            else if (thread != x) conflict = 1;
        }
        out->row_thread[t] = conflict ? -1 : thread;
        out->row_conflict[t] = conflict;
    }
    free(next); free(occurs); free(linked);
    return PWR_OK;
fail:
    free(next); free(occurs); free(linked);
    pgr_threads_free(out);
    return rc;
}

/* Resolvability (TransposonAssessment.py:97-119, "TA:") on the diff matrix of pgr_msa_consensus */
int pgr_resolvability(int parts, const int *diff, int *unique11, int *min_diff, int *last_diff)
{
    if (parts < 2 || !diff || !unique11 || !min_diff || !last_diff) return PWR_ERR_ARG;   /* (TA:112 reads a `diff` never set) */
    for (int t = 0; t < 11; t++) unique11[t] = 0;
    for (int k = 0; k < parts; k++) {
        int mindiff = 1000000, last = 0;                                              /* TA:104 */
        for (int kk = 0; kk < parts; kk++) {
            if (kk == k) continue;
            last = diff[(size_t)k * parts + kk];                                      /* TA:107 */
            if (last < mindiff) mindiff = last;
        }
        for (int t = 0; t < 11; t++) unique11[t] += mindiff > t;                      /* TA:110-114: unique[t] survives while every diff > t */
        min_diff[k] = mindiff;
        last_diff[k] = last;                                                          /* TA:112 appends diff, not mindiff */
    }
    return PWR_OK;
}
