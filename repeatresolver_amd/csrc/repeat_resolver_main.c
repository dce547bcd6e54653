/* Drop-in for the reference's `RepeatResolver` (RepeatResolver.c main(), RR:3863-4084): same argv, reads MaxCorrsOf_<MApath>
 * from the current directory and writes the reference's three label files, DropoffSubdivisionOf_, RelDropSubdivisionOf_ and
 * KmeansSubdivisionOf_<von>_<bis>_<MApath>.  The refinement, stage 2 and the k-means stage run on the GPU behind
 * include/pgr.h.  -p and -o are accepted and ignored.  Extra flag: -g <device>.
 * Undefined in the reference, defined here: a missing MaxCorrsOf_ file (the reference dereferences NULL, RR:3981; its own
 * AllMaxCorrsRechner behind RR:3987 is never reached) prints a message and exits 1, as does any other failure. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pgr.h"

static int fail(const char *what, int rc)
{
    printf("RepeatResolver: %s: %s\n", what, pwr_strerror(rc));
    return 1;
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("Usage: ./RepeatResolver MApath <options>\n"); return 0; }      /* RR:3869 */
    const char *msa = argv[1];
    int cov = 30, von = -1, bis = -1, device = 0;                                           /* RR:3872-3878 */
    double cutoff = 0.0;
    for (int i = 2; i < argc; i++) {
        if (argv[i][0] != '-') continue;
        if (argv[i][1] == 'p' && i + 1 < argc) printf("NTHREADS: %ld\n", strtol(argv[i + 1], NULL, 10));       /* RR:3896-3897 */
        if (argv[i][1] == 'h') { printf("Usage: ./RepeatResolver MApath -c coverage -f from until -t threshold\n"); return 0; }
        if (argv[i][1] == 'c' && i + 1 < argc) { cov = (int)strtol(argv[i + 1], NULL, 10); printf("Coverage %d\n", cov); }
        if (argv[i][1] == 'f' && i + 2 < argc) {                                            /* RR:3927-3932 */
            von = (int)strtol(argv[i + 1], NULL, 10); bis = (int)strtol(argv[i + 2], NULL, 10);
            printf("Full coverage from column %d until %d.\n", von, bis);
        }
        if (argv[i][1] == 't' && i + 1 < argc) cutoff = atof(argv[i + 1]);                  /* RR:3942 */
        if (argv[i][1] == 'g' && i + 1 < argc) device = atoi(argv[i + 1]);
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
    if ((rc = pwr_read_msa_file(msa, &rows, &width, &text, err, sizeof err))) { printf("%s\n", err); return 1; }
    if (snprintf(name, sizeof name, "MaxCorrsOf_%s", msa) >= (int)sizeof name) { free(text); return fail(msa, PWR_ERR_RANGE); }   /* RR:3967-3968 */
    printf("%s\n", name);
    if ((rc = pgr_read_maxcorrs_file(name, 0, width - 1, &mc, &n))) {
        if (rc == PWR_ERR_INPUT) printf("RepeatResolver: %s is missing: run MaxCorrelation on %s first.\n", name, msa);
        else fail(name, rc);
        free(text);
        return 1;
    }
    if (n != width * 5) { printf("RepeatResolver: %s holds %d values, the MSA has %d variations.\n", name, n, width * 5); goto done; }
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
    free(mc); free(text);
    return status;
}
