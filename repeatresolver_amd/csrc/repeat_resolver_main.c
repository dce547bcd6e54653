/* Drop-in for the reference's `RepeatResolver` (RepeatResolver.c main(), RR:3863-4084): same argv, reads MaxCorrsOf_<MApath>
 * from the current directory and writes the reference's three label files, DropoffSubdivisionOf_, RelDropSubdivisionOf_ and
 * KmeansSubdivisionOf_<von>_<bis>_<MApath>.  The refinement, stage 2 and the k-means stage run on the GPU behind
 * include/pgr.h.  -p and -o are accepted and ignored.  Extra flags: -g <device>, and
 *   -w s0 s1 ... sn   (the integers up to the next argument that begins with '-'; at least two, strictly increasing): the
 *                     windows [s0, s1], [s1, s2], ... in one run, as the reference README's sequence `-f s0 s1`, `-f s1 s2`,
 *                     ... -- the MSA and the MaxCorrs file are read once, the MSA goes to the device once
 *                     (pgr_msa_resolve), every window's three label files are written under the names and with the bytes of
 *                     its -f run, and ConnectionsOf_<s0>_<sn>_<MApath> holds the connection matrix of the windows' k-means
 *                     labels (pgr_connect): "<K_first> <K_last>", then K_first lines of K_last values in %f.  With -w a
 *                     missing MaxCorrsOf_ file is computed (pmc_maxcorrs at the -c coverage), written and read back, as
 *                     RR:3987-3999 intends.
 *   -l <FlankingLeft> -r <FlankingRight>   (with -w, both or neither): two labellings of the MSA's rows, one integer per line
 *                     (FlankClusterer writes them, include/pfl.h).  They go in front of and behind the windows' k-means labels
 *                     into pgr_connect, as SDA:375 puts them, and ConnectionsOf_ is then the matrix from the left flanks'
 *                     clusters to the right flanks'.  Without them nothing changes.
 * Undefined in the reference, defined here: a missing MaxCorrsOf_ file (the reference dereferences NULL, RR:3981; its own
 * AllMaxCorrsRechner behind RR:3987 is never reached) prints a message and exits 1, as does any other failure. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pgr.h"
#include "pmc.h"

static int fail(const char *what, int rc)
{
    printf("RepeatResolver: %s: %s\n", what, pwr_strerror(rc));
    return 1;
}

/* a labelling of the MSA's rows from a file of one integer per line (pfl_write_labels) */
static int read_labels(const char *path, int rows, int *out)
{
    FILE *f = fopen(path, "r");
    int n = 0, v;
    if (!f) return PWR_ERR_INPUT;
    while (fscanf(f, "%d", &v) == 1) {
        if (n == rows || v < -1) { fclose(f); return PWR_ERR_INPUT; }
        out[n++] = v;
    }
    fclose(f);
    return n == rows ? PWR_OK : PWR_ERR_INPUT;
}

/* -w: the windows of sites[nsites] in one call; returns the exit code */
static int run_windows(const char *msa, int rows, int width, const unsigned char *text, const double *mc, int nsites, const int *sites,
                       int cov, double cutoff, int device, const char *flank_left, const char *flank_right)
{
    pgr_msa *h = NULL;
    pgr_resolution rs;
    pgr_connection cn;
    char name[600];
    int rc, status = 1;
    memset(&rs, 0, sizeof rs); memset(&cn, 0, sizeof cn);
    if ((rc = pgr_msa_open(rows, width, text, device, &h))) return fail("MSA to the device", rc);
    if ((rc = pgr_msa_resolve(h, mc, nsites, sites, cov, cutoff, &rs))) { fail("resolution", rc); goto done; }
    for (int p = 0; p < rs.nwindows; p++) {
        const pgr_resolved_window *w = rs.windows + p;
        const char *stage[3] = {"Dropoff", "RelDrop", "Kmeans"};
        const int *labels[3] = {w->dropoff_labels, w->reldrop_labels, w->kmeans_labels};
        printf("Full coverage from column %d until %d.\n", w->von, w->bis);
        printf("Cutoff %f\n", w->cutoff);
        for (int s = 0; s < 3; s++) {
            if ((rc = pgr_subdivision_name(name, sizeof name, stage[s], w->von, w->bis, msa))) { fail("file name", rc); goto done; }
            if ((rc = pgr_write_subdivision(name, labels[s], rows))) { fail(name, rc); goto done; }
        }
        printf("Parts: %d, %d, %d\n", w->dropoff_parts, w->reldrop_parts, w->kmeans_parts);
    }
    {
        const int fl = flank_left ? 1 : 0;                                          /* a labelling in front and one behind */
        int *all = malloc(sizeof(int) * (size_t)(rs.nwindows + 2 * fl) * (size_t)rows);
        if (!all) { fail("connections", PWR_ERR_NOMEM); goto done; }
        for (int p = 0; p < rs.nwindows; p++) memcpy(all + (size_t)(p + fl) * rows, rs.windows[p].kmeans_labels, sizeof(int) * (size_t)rows);
        if (fl) {
            if ((rc = read_labels(flank_left, rows, all))) { fail(flank_left, rc); free(all); goto done; }
            if ((rc = read_labels(flank_right, rows, all + (size_t)(rs.nwindows + 1) * rows))) { fail(flank_right, rc); free(all); goto done; }
        }
        if (rs.nwindows + 2 * fl < 2) { printf("One window: no connections.\n"); free(all); status = 0; goto done; }
        rc = pgr_connect(rs.nwindows + 2 * fl, rows, all, &cn);
        free(all);
        if (rc) { fail("connections", rc); goto done; }
    }
    if (snprintf(name, sizeof name, "ConnectionsOf_%d_%d_%s", sites[0], sites[nsites - 1], msa) >= (int)sizeof name) { fail(msa, PWR_ERR_RANGE); goto done; }
    {
        FILE *f = fopen(name, "w");
        if (!f) { fail(name, PWR_ERR_IO); goto done; }
        fprintf(f, "%d %d\n", cn.k_first, cn.k_last);
        for (int a = 0; a < cn.k_first; a++) {
            for (int b = 0; b < cn.k_last; b++) fprintf(f, b ? " %f" : "%f", cn.matrix[(size_t)a * cn.k_last + b]);
            fprintf(f, "\n");
        }
        if (fclose(f) != 0) { fail(name, PWR_ERR_IO); goto done; }
    }
    printf("Connections: %d x %d\n", cn.k_first, cn.k_last);
    status = 0;
done:
    pgr_connection_free(&cn); pgr_resolution_free(&rs); pgr_msa_close(h);
    return status;
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("Usage: ./RepeatResolver MApath <options>\n"); return 0; }      /* RR:3869 */
    const char *msa = argv[1];
    int cov = 30, von = -1, bis = -1, device = 0;                                           /* RR:3872-3878 */
    int nsites = 0, windows = 0;
    int *sites = calloc((size_t)argc, sizeof(int));
    double cutoff = 0.0;
    const char *flank_left = NULL, *flank_right = NULL;
    if (!sites) return fail("arguments", PWR_ERR_NOMEM);
    for (int i = 2; i < argc; i++) {
        if (argv[i][0] != '-') continue;
        if (argv[i][1] == 'p' && i + 1 < argc) printf("NTHREADS: %ld\n", strtol(argv[i + 1], NULL, 10));       /* RR:3896-3897 */
        if (argv[i][1] == 'h') { printf("Usage: ./RepeatResolver MApath -c coverage -f from until -t threshold\n"); free(sites); return 0; }
        if (argv[i][1] == 'c' && i + 1 < argc) { cov = (int)strtol(argv[i + 1], NULL, 10); printf("Coverage %d\n", cov); }
        if (argv[i][1] == 'f' && i + 2 < argc) {                                            /* RR:3927-3932 */
            von = (int)strtol(argv[i + 1], NULL, 10); bis = (int)strtol(argv[i + 2], NULL, 10);
            printf("Full coverage from column %d until %d.\n", von, bis);
        }
        if (argv[i][1] == 't' && i + 1 < argc) cutoff = atof(argv[i + 1]);                  /* RR:3942 */
        if (argv[i][1] == 'g' && i + 1 < argc) device = atoi(argv[i + 1]);
        if (argv[i][1] == 'l' && i + 1 < argc) flank_left = argv[i + 1];
        if (argv[i][1] == 'r' && i + 1 < argc) flank_right = argv[i + 1];
        if (argv[i][1] == 'w') {
            windows = 1; nsites = 0;
            for (int j = i + 1; j < argc && argv[j][0] != '-'; j++) {
                char *end;
                const long v = strtol(argv[j], &end, 10);
                if (*end || end == argv[j] || v > PGR_MAX_COLUMNS || (nsites > 0 && v <= sites[nsites - 1])) {
                    printf("RepeatResolver: -w takes strictly increasing column numbers, not \"%s\".\n", argv[j]);
                    free(sites);
                    return 1;
                }
                sites[nsites++] = (int)v;
            }
        }
    }
    if (windows && nsites < 2) { printf("RepeatResolver: -w needs at least two column numbers.\n"); free(sites); return 1; }
    if ((flank_left || flank_right) && !(windows && flank_left && flank_right)) {
        printf("RepeatResolver: -l and -r go together, and with -w.\n");
        free(sites);
        return 1;
    }
    int rows = 0, width = 0, n = 0, rc, status = 1;
    unsigned char *text = NULL;
    double *mc = NULL;
    char err[200] = "", name[600];
    pgr_window win;
    pgr_result res;
    pgr_subdivision sd;
    pgr_kmeans km;
    memset(&win, 0, sizeof win); memset(&res, 0, sizeof res); memset(&sd, 0, sizeof sd); memset(&km, 0, sizeof km);
    if ((rc = pwr_read_msa_file(msa, &rows, &width, &text, err, sizeof err))) { printf("%s\n", err); free(sites); return 1; }
    if (snprintf(name, sizeof name, "MaxCorrsOf_%s", msa) >= (int)sizeof name) { free(text); free(sites); return fail(msa, PWR_ERR_RANGE); }   /* RR:3967-3968 */
    printf("%s\n", name);
    rc = pgr_read_maxcorrs_file(name, 0, width - 1, &mc, &n);
    if (rc == PWR_ERR_INPUT && windows) {                                                   /* RR:3987-3999, as intended */
        double *made = malloc(sizeof(double) * (size_t)width * 5);
        printf("RepeatResolver: %s is missing: computing it at coverage %d.\n", name, cov);
        if (!made) rc = PWR_ERR_NOMEM;
        else if (!(rc = pmc_maxcorrs(rows, width, text, cov, device, made)) && !(rc = pmc_write(name, width * 5, made)))
            rc = pgr_read_maxcorrs_file(name, 0, width - 1, &mc, &n);                       /* the values later runs will read */
        free(made);
        if (rc) { fail(name, rc); free(text); free(sites); return 1; }
    }
    if (rc) {
        if (rc == PWR_ERR_INPUT) printf("RepeatResolver: %s is missing: run MaxCorrelation on %s first.\n", name, msa);
        else fail(name, rc);
        free(text); free(sites);
        return 1;
    }
    if (n != width * 5) { printf("RepeatResolver: %s holds %d values, the MSA has %d variations.\n", name, n, width * 5); goto done; }
    if (windows) { status = run_windows(msa, rows, width, text, mc, nsites, sites, cov, cutoff, device, flank_left, flank_right); goto done; }
    if ((rc = pgr_refine(rows, width, text, mc, von, bis, cov, cutoff, device, &res))) { fail("group refinement", rc); goto done; }
    printf("Cutoff %f\n", res.cutoff);                                                      /* RR:3984 */
    if ((rc = pgr_read_window(rows, width, text, von, bis, &win))) { fail("window", rc); goto done; }
    if ((rc = pgr_subdivide(&win, &res, cov, device, &sd))) { fail("subdivision", rc); goto done; }
    if ((rc = pgr_kmeans_subdivide(&win, &res, sd.reldrop_labels, cov, device, &km))) { fail("k-means subdivision", rc); goto done; }
    {
        const char *stage[3] = {"Dropoff", "RelDrop", "Kmeans"};
        const int *labels[3] = {sd.dropoff_labels, sd.reldrop_labels, km.labels};
        for (int s = 0; s < 3; s++) {                                                       /* RR:4040-4075 */
            if ((rc = pgr_subdivision_name(name, sizeof name, stage[s], von, bis, msa))) { fail("file name", rc); goto done; }
            if ((rc = pgr_write_subdivision(name, labels[s], rows))) { fail(name, rc); goto done; }
        }
    }
    printf("Parts: %d, %d, %d\n", sd.dropoff_parts, sd.reldrop_parts, km.parts);
    status = 0;
done:
    pgr_kmeans_free(&km); pgr_subdivision_free(&sd); pgr_window_free(&win); pgr_free(&res);
    free(mc); free(text); free(sites);
    return status;
}
