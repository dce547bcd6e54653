/* pgr_host.c -- host side of RepeatResolver's group refinement, plain C: the window reader, the MaxCorrs slice and the
 * preparation in main() (RR:293-429, RR:609-646, RR:3977-4014). */
#define _POSIX_C_SOURCE 200809L
#include "pgr.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int code_of(unsigned char ch)
{
    switch (ch) {                                                                  /* RR:336-359 */
    case 'a': case 'A': return 0;
    case 'c': case 'C': return 1;
    case 'g': case 'G': return 2;
    case 't': case 'T': return 3;
    case '-': case '_': return 4;
    default: return 5;
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
            const int k = code_of(line[i]);
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
