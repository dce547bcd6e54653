/* TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The host side of the locus anchorer (repeatresolver_amd/csrc/pla_host.c: the two
 * readers, pla_place, the two writers, the frees on the failure paths) under the host sanitizers, as a program of its own.
 * Every buffer handed in is allocated at exactly the size the header promises, so a byte too many is a report.  The entries
 * of other files that pla_host.c calls are stubs here: only pla_run_files reaches them, and it is run up to the point where it
 * would open the device.  From the repository's root:
 *   cc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *      tests/anchor_sanitize_main.c repeatresolver_amd/csrc/pla_host.c -o anchor_sanitize && ./anchor_sanitize <a directory to write in>
 * It prints one line and returns 0 when every check holds; a sanitizer report ends it with a non-zero status.
 * tests/test_anchors.py builds and runs it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pla.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

/* what pla_host.c links against elsewhere in the library */
int pla_create(pla_ctx **out, int device) { (void)out; (void)device; return PWR_ERR_DEVICE; }
void pla_destroy(pla_ctx *c) { (void)c; }
int pla_open_text(pla_ctx *c, int nc, const char *b, const long long *o) { (void)c; (void)nc; (void)b; (void)o; return PWR_ERR_DEVICE; }
int pla_search(pla_ctx *c, int np, const char *a, const long long *o, const int *s, int reach, int min_len, int pm, pla_hits *out)
{
    (void)c; (void)np; (void)a; (void)o; (void)s; (void)reach; (void)min_len; (void)pm; (void)out;
    return PWR_ERR_DEVICE;
}
int pla_get_stats(pla_ctx *c, unsigned long long *cells, double *ms) { (void)c; (void)cells; (void)ms; return PWR_ERR_DEVICE; }
const char *pwr_strerror(int rc) { (void)rc; return "stub"; }

static char dir[4000];

static const char *in_dir(const char *name)
{
    static char path[4200];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    return path;
}

static int put(const char *name, const char *text)
{
    FILE *f = fopen(in_dir(name), "w");
    if (!f) return 1;
    fputs(text, f);
    return fclose(f);
}

static int file_is(const char *name, const char *want)
{
    FILE *f = fopen(in_dir(name), "r");
    if (!f) return 0;
    const size_t n = strlen(want);
    char *got = malloc(n + 2);
    const size_t k = fread(got, 1, n + 1, f);
    fclose(f);
    const int same = k == n && memcmp(got, want, n) == 0;
    free(got);
    return same;
}

/* hits in exactly sized arrays */
static int make_hits(int n, const int (*rows)[7], pla_hits *h)
{
    int **f[7] = {&h->pattern, &h->orientation, &h->contig, &h->boundary, &h->lo, &h->hi, &h->distance};
    memset(h, 0, sizeof *h);
    h->n = n;
    for (int k = 0; k < 7; k++) {
        *f[k] = malloc(sizeof(int) * (size_t)(n ? n : 1));
        if (!*f[k]) return 1;
        for (int i = 0; i < n; i++) (*f[k])[i] = rows[i][k];
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || strlen(argv[1]) >= sizeof dir) { fprintf(stderr, "usage: anchor_sanitize <directory>\n"); return 2; }
    strcpy(dir, argv[1]);

    /* ---- pla_read_contigs ---- */
    pla_contigs c;
    CHECK(put("a.fasta", ">one first contig\nacgtNN\nACGTry\n\n>two\n>three\tx\r\nac gt\r\nnnnn-*\n>\nA") == 0);
    CHECK(pla_read_contigs(in_dir("a.fasta"), &c) == PWR_OK);
    CHECK(c.nc == 4 && !strcmp(c.name[0], "one") && !strcmp(c.name[1], "two") && !strcmp(c.name[2], "three") && !strcmp(c.name[3], ""));
    CHECK(c.off[0] == 0 && c.off[1] == 12 && c.off[2] == 12 && c.off[3] == 22 && c.off[4] == 23);
    CHECK(memcmp(c.bases, "acgtnnACGTnnacgtnnnnnnA", 23) == 0);
    pla_contigs_free(&c);
    pla_contigs_free(&c);                                                           /* (zeroed: a second free is harmless) */
    {   /* many records and a long one: every growth path of the reader */
        FILE *f = fopen(in_dir("big.fasta"), "w");
        CHECK(f != NULL);
        for (int j = 0; j < 70; j++) {
            fprintf(f, ">contig_with_a_rather_long_name_to_grow_the_header_buffer_beyond_its_first_sixty_four_bytes_%d and more\n", j);
            for (int x = 0; x < (j == 3 ? 200000 : j); x++) { fputc("acgtN"[x % 5], f); if (x % 60 == 59) fputc('\n', f); }
            fputc('\n', f);
        }
        CHECK(fclose(f) == 0);
        CHECK(pla_read_contigs(in_dir("big.fasta"), &c) == PWR_OK);
        CHECK(c.nc == 70 && c.off[4] - c.off[3] == 200000 && c.off[70] == 200000 + 69 * 70 / 2 - 3 && c.bases[c.off[3] + 4] == 'n');
        CHECK(strlen(c.name[69]) > 64);
        pla_contigs_free(&c);
    }
    CHECK(put("empty.fasta", "") == 0);
    CHECK(pla_read_contigs(in_dir("empty.fasta"), &c) == PWR_OK && c.nc == 0);
    pla_contigs_free(&c);
    CHECK(put("bad.fasta", "acgt\n>x\nac\n") == 0);
    CHECK(pla_read_contigs(in_dir("bad.fasta"), &c) == PWR_ERR_INPUT && c.nc == 0 && !c.bases);
    CHECK(pla_read_contigs(in_dir("missing.fasta"), &c) == PWR_ERR_IO && pla_read_contigs(NULL, &c) == PWR_ERR_ARG);
    CHECK(pla_read_contigs(in_dir("a.fasta"), NULL) == PWR_ERR_ARG);

    /* ---- pla_read_loci ---- */
    pla_loci l;
    CHECK(put("l.fasta", ">toy_locus0 left=3:5 copy=4 right=7:3 rows=5\nACGTTGGGGCCA\n>toy_locus1 left=-1:0 copy=4 right=2:4 rows=5\nACACTTTG\n"
                         ">toy_locus2 left=4:2 copy=1 right=0:0 rows=5\nACG\n") == 0);
    CHECK(pla_read_loci(in_dir("l.fasta"), &l) == PWR_OK && l.n == 3);
    CHECK(!strcmp(l.name[0], "toy_locus0") && !strcmp(l.name[2], "toy_locus2"));
    CHECK(l.left_len[0] == 5 && l.copy_len[0] == 4 && l.right_len[0] == 3 && l.left_len[1] == 0 && l.right_len[2] == 0);
    CHECK(l.aoff[0] == 0 && l.aoff[1] == 5 && l.aoff[2] == 8 && l.aoff[3] == 8 && l.aoff[4] == 12 && l.aoff[5] == 14 && l.aoff[6] == 14);
    CHECK(memcmp(l.anchored, "TTGCACCATTTGCA", 14) == 0 && l.side[0] == 0 && l.side[5] == 1);
    pla_loci_free(&l);
    pla_loci_free(&l);
    CHECK(put("l2.fasta", ">x left=1:2 copy=1 right=1:1\nACG\n") == 0);            /* the lengths do not add up */
    CHECK(pla_read_loci(in_dir("l2.fasta"), &l) == PWR_ERR_INPUT && l.n == 0 && !l.seq);
    CHECK(put("l3.fasta", ">ok left=1:1 copy=1 right=1:1\nACG\n>x left=1:1 copy=1\nACG\n") == 0);   /* a field is missing, after a good record */
    CHECK(pla_read_loci(in_dir("l3.fasta"), &l) == PWR_ERR_INPUT && l.n == 0 && !l.name);
    CHECK(put("l4.fasta", ">x left=1:1 copy=1 right=1:1\nANG\n") == 0);            /* a byte that is no base */
    CHECK(pla_read_loci(in_dir("l4.fasta"), &l) == PWR_ERR_INPUT);
    CHECK(put("l5.fasta", ">xleft=9:9 left=1:1 notcopy=7 copy=1 right=1:1\nACG\n") == 0);   /* keys are whole words */
    CHECK(pla_read_loci(in_dir("l5.fasta"), &l) == PWR_OK && l.left_len[0] == 1 && l.copy_len[0] == 1);
    pla_loci_free(&l);
    CHECK(pla_read_loci(in_dir("missing.fasta"), &l) == PWR_ERR_IO && pla_read_loci(NULL, &l) == PWR_ERR_ARG);

    /* ---- pla_place and the writers ---- */
    static const int rows[9][7] = {{0, 0, 0, 5, 5, 5, 1}, {1, 0, 0, 10, 10, 10, 2}, {2, 1, 0, 20, 20, 20, 0}, {3, 1, 0, 15, 15, 15, 0},
                                   {4, 0, 1, 4, 4, 4, 0}, {5, 0, 1, 4, 4, 4, 0}, {6, 0, 1, 8, 8, 8, 0}, {7, 0, 0, 22, 22, 22, 0},
                                   {8, 1, 1, 11, 11, 11, 0}};
    pla_hits h;
    CHECK(make_hits(9, rows, &h) == 0);
    int *lp = malloc(sizeof(int) * 6), *rp = malloc(sizeof(int) * 6);
    pla_placement *pl = malloc(sizeof(pla_placement) * 6);
    CHECK(lp && rp && pl);
    for (int i = 0; i < 6; i++) { lp[i] = 2 * i; rp[i] = 2 * i + 1; }
    CHECK(pla_place(6, lp, rp, &h, 10, pl) == PWR_OK);
    CHECK(pl[0].status == PLA_PLACED && pl[1].status == PLA_PLACED && pl[2].status == PLA_PLACED && pl[3].status == PLA_BRIDGE &&
          pl[4].status == PLA_LEFT_ONLY && pl[5].status == PLA_NONE);
    CHECK(pl[1].lo == 15 && pl[1].hi == 20 && pl[1].span == 5 && pl[1].has_span && pl[2].span == 0 && !pl[3].has_span && pl[3].lo == -1);
    CHECK(pla_place(6, lp, rp, &h, -1, pl) == PWR_ERR_ARG && pla_place(6, NULL, rp, &h, 10, pl) == PWR_ERR_ARG && pla_place(6, lp, rp, NULL, 10, pl) == PWR_ERR_ARG);
    CHECK(pla_place(0, NULL, NULL, &h, 10, NULL) == PWR_OK);
    CHECK(put("c.fasta", ">c0\naaaaaCCCCCgggggTTTTTnnnnn\n>c1\nacgtacgtacgt\n>c2\n") == 0);
    CHECK(pla_read_contigs(in_dir("c.fasta"), &c) == PWR_OK && c.nc == 3);
    const char *names[6] = {"t_locus0", "t_locus1", "t_locus2", "t_locus3", "t_locus4", "t_locus5"};
    CHECK(pla_write_placements(in_dir("p"), 6, names, pl, &c) == PWR_OK);
    CHECK(file_is("p", "t_locus0\tPLACED\tc0\tc0\t+\t+\t5\t10\t5\t10\t5\t1\t2\n"
                       "t_locus1\tPLACED\tc0\tc0\t-\t-\t20\t15\t15\t20\t5\t0\t0\n"
                       "t_locus2\tPLACED\tc1\tc1\t+\t+\t4\t4\t4\t4\t0\t0\t0\n"
                       "t_locus3\tBRIDGE\tc1\tc0\t+\t+\t8\t22\t-\t-\t-\t0\t0\n"
                       "t_locus4\tLEFT_ONLY\tc1\t-\t-\t-\t11\t-\t-\t-\t-\t0\t-\n"
                       "t_locus5\tNONE\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n"));
    char *copies = malloc(16);                                                      /* ACGTA AAACG tt GGGG and two empty ones: exactly 16 bytes */
    long long *coff = malloc(sizeof(long long) * 7);
    CHECK(copies && coff);
    memcpy(copies, "ACGTAAAACGttGGGGC", 16);
    { const long long o[7] = {0, 5, 10, 12, 16, 16, 16}; memcpy(coff, o, sizeof o); }
    CHECK(pla_write_patched(in_dir("f"), &c, 6, pl, copies, coff) == PWR_OK);
    CHECK(file_is("f", ">c0 patched=2\naaaaaACGTAgggggCGTTTnnnnn\n>c1 patched=1\nacgtttacgtacgt\n>c2 patched=0\n\n"));
    /* refusals of the writers: an interval beyond its contig, descending offsets, a contig that is not there, a path that cannot be opened */
    pl[0].hi = 26;
    CHECK(pla_write_patched(in_dir("f2"), &c, 6, pl, copies, coff) == PWR_ERR_ARG);
    pl[0].hi = 10;
    coff[2] = 4;
    CHECK(pla_write_patched(in_dir("f2"), &c, 6, pl, copies, coff) == PWR_ERR_ARG);
    coff[2] = 10;
    pl[4].left_contig = 3;
    CHECK(pla_write_placements(in_dir("p2"), 6, names, pl, &c) == PWR_ERR_ARG);
    pl[4].left_contig = 1;
    CHECK(pla_write_placements(in_dir("no/such/dir/p"), 6, names, pl, &c) == PWR_ERR_IO);
    CHECK(pla_write_patched(in_dir("no/such/dir/f"), &c, 6, pl, copies, coff) == PWR_ERR_IO);
    CHECK(pla_write_patched(in_dir("f3"), &c, 0, NULL, NULL, NULL) == PWR_OK);
    CHECK(file_is("f3", ">c0 patched=0\naaaaaCCCCCgggggTTTTTnnnnn\n>c1 patched=0\nacgtacgtacgt\n>c2 patched=0\n\n"));
    /* conflicts: [5, 10) and [9, 12) of c0 */
    static const int clash[4][7] = {{0, 0, 0, 5, 5, 5, 0}, {1, 0, 0, 10, 10, 10, 0}, {2, 0, 0, 9, 9, 9, 0}, {3, 0, 0, 12, 12, 12, 0}};
    pla_hits h2;
    CHECK(make_hits(4, clash, &h2) == 0);
    CHECK(pla_place(2, lp, rp, &h2, 10, pl) == PWR_OK && pl[0].status == PLA_CONFLICT && pl[1].status == PLA_CONFLICT);
    pla_hits_free(&h2);
    pla_hits_free(&h2);
    /* the drop-in's run, as far as it goes without a device: everything read and prepared, then freed on the failure path */
    char prefix[4200];
    snprintf(prefix, sizeof prefix, "%s/run", dir);
    FILE *log = fopen(in_dir("log"), "w");
    CHECK(log != NULL);
    char lpath[4200];
    snprintf(lpath, sizeof lpath, "%s", in_dir("l.fasta"));
    CHECK(pla_run_files(lpath, in_dir("c.fasta"), 100, 50, 256, 1, prefix, 0, log) == 1);       /* the stub has no device */
    CHECK(pla_run_files(lpath, in_dir("missing.fasta"), 100, 50, 256, 1, prefix, 0, log) == 1);
    CHECK(pla_run_files(in_dir("l2.fasta"), in_dir("c.fasta"), 100, 50, 256, 1, prefix, 0, log) == 1);
    CHECK(pla_run_files(lpath, in_dir("c.fasta"), 100, -1, 256, 1, prefix, 0, log) == 1 && pla_run_files(NULL, NULL, 0, 0, 0, 0, NULL, 0, NULL) == 1);
    CHECK(fclose(log) == 0);
    pla_contigs_free(&c);
    pla_hits_free(&h);
    free(lp); free(rp); free(pl); free(copies); free(coff);
    printf("anchor_sanitize: ok\n");
    return 0;
}
