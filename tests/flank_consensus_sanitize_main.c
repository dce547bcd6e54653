/* TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The host side of the flank consensus that has index arithmetic of its own (pfl_call, the
 * compaction of the votes; pfl_consensus_pack, what pfl_consensus ends with; pfl_write_flank_fasta; pfl_consensus_free; repeatresolver_amd/csrc/pfl_host.c) under the host sanitizers,
 * as a program of its own.  Every buffer is allocated at exactly the size the header promises, so a byte too many is a report.
 * The entries of other files that pfl_host.c calls are stubs here: nothing below reaches them.  From the repository's root:
 *   cc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *      tests/flank_consensus_sanitize_main.c repeatresolver_amd/csrc/pfl_host.c -o flank_consensus_sanitize && ./flank_consensus_sanitize
 * It prints one line and returns 0 when every check holds; a sanitizer report ends it with a non-zero status. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfl.h"
#include "pia.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

/* what pfl_host.c links against elsewhere in the library */
int pfl_create(pfl_ctx **out, int device) { (void)out; (void)device; return PWR_ERR_DEVICE; }
void pfl_destroy(pfl_ctx *c) { (void)c; }
int pfl_get_stats(pfl_ctx *c, unsigned long long *cells, double *ms) { (void)c; (void)cells; (void)ms; return PWR_ERR_DEVICE; }
int pfl_distances(pfl_ctx *c, int n, const char *b, const long long *o, const int *p, const int *m, int reach, int min_len, int *len,
                  int *dist)
{
    (void)c; (void)n; (void)b; (void)o; (void)p; (void)m; (void)reach; (void)min_len; (void)len; (void)dist;
    return PWR_ERR_DEVICE;
}
int pfl_consensus(pfl_ctx *c, int n, const char *b, const long long *o, const int *p, const int *m, const int *l, int block, int extent,
                  int max_permille, int min_depth, int rounds, pfl_consensus_result *out)
{
    (void)c; (void)n; (void)b; (void)o; (void)p; (void)m; (void)l; (void)block; (void)extent; (void)max_permille; (void)min_depth;
    (void)rounds; (void)out;
    return PWR_ERR_DEVICE;
}
int pia_read_fasta(const char *path, int *n, char **bases, long long **off) { (void)path; (void)n; (void)bases; (void)off; return PWR_ERR_IO; }
const char *pwr_strerror(int rc) { (void)rc; return "stub"; }

/* pfl_call on buffers of exactly npos and 2 * npos entries, against the rule restated here */
static int call_case(int npos, const unsigned char *sym_in, const unsigned char *ins_in, const int *voters_in, int min_depth,
                     const char *want, const int *want_depth)
{
    unsigned char *sym = calloc((size_t)npos + !npos, 1), *ins = calloc((size_t)npos + !npos, 1);
    int *voters = calloc((size_t)npos + !npos, sizeof(int)), *depth = malloc(sizeof(int) * ((size_t)npos * 2 + !npos));
    char *seq = malloc((size_t)npos * 2 + !npos);
    CHECK(sym && ins && voters && depth && seq);
    if (npos) { memcpy(sym, sym_in, (size_t)npos); memcpy(ins, ins_in, (size_t)npos); memcpy(voters, voters_in, sizeof(int) * (size_t)npos); }
    const int got = pfl_call(npos, sym, ins, voters, min_depth, seq, depth);
    int exp = 0;
    for (int i = 0; i < npos && voters_in[i] >= min_depth; i++) exp += (sym_in[i] < 4) + (ins_in[i] != 0);
    CHECK(got == exp && got <= 2 * npos);
    if (want) {
        CHECK(got == (int)strlen(want) && memcmp(seq, want, (size_t)got) == 0);
        for (int k = 0; k < got; k++) CHECK(depth[k] == want_depth[k]);
    }
    int k = 0;
    for (int i = 0; i < npos && voters_in[i] >= min_depth; i++) {
        if (sym_in[i] < 4) { CHECK(seq[k] == "acgt"[sym_in[i]] && depth[k] == voters_in[i]); k++; }
        if (ins_in[i]) { CHECK(seq[k] == "acgt"[ins_in[i] - 1] && depth[k] == voters_in[i]); k++; }
    }
    CHECK(k == got);
    free(sym); free(ins); free(voters); free(depth); free(seq);
    return 0;
}

static int fasta_case(const char *path)
{
    /* three clusters: 5 bases, none, 1 base; allocated as pfl_consensus allocates them */
    pfl_consensus_result r;
    memset(&r, 0, sizeof r);
    r.nclusters = 3;
    r.label = malloc(sizeof(int) * 3); r.members = malloc(sizeof(int) * 3); r.backbone = malloc(sizeof(int) * 3);
    r.off = malloc(sizeof(long long) * 4); r.seq = malloc(7); r.depth = malloc(sizeof(int) * 6);
    CHECK(r.label && r.members && r.backbone && r.off && r.seq && r.depth);
    const int label[3] = {0, 4, 11}, members[3] = {7, 0, 2}, backbone[3] = {3, -1, 9};
    memcpy(r.label, label, sizeof label); memcpy(r.members, members, sizeof members); memcpy(r.backbone, backbone, sizeof backbone);
    r.off[0] = 0; r.off[1] = 5; r.off[2] = 5; r.off[3] = 6;
    memcpy(r.seq, "aacgtc", 7);
    for (int k = 0; k < 6; k++) r.depth[k] = 2;
    char text[256];
    for (int side = 0; side < 2; side++) {
        CHECK(pfl_write_flank_fasta(path, side ? "right" : "left", &r) == PWR_OK);
        FILE *f = fopen(path, "r");
        CHECK(f);
        const size_t n = fread(text, 1, sizeof text - 1, f);
        fclose(f);
        text[n] = 0;
        const char *want = side ? ">right_0 flanks=7 bases=5\nAACGT\n>right_4 flanks=0 bases=0\n\n>right_11 flanks=2 bases=1\nC\n"
                                : ">left_0 flanks=7 bases=5\nTGCAA\n>left_4 flanks=0 bases=0\n\n>left_11 flanks=2 bases=1\nC\n";
        CHECK(strcmp(text, want) == 0);
    }
    CHECK(pfl_write_flank_fasta(path, "middle", &r) == PWR_ERR_ARG && pfl_write_flank_fasta(NULL, "left", &r) == PWR_ERR_ARG);
    CHECK(pfl_write_flank_fasta(path, "left", NULL) == PWR_ERR_ARG);
    CHECK(pfl_write_flank_fasta("/nonexistent-directory/x.fasta", "left", &r) == PWR_ERR_IO);
    pfl_consensus_free(&r);
    CHECK(r.nclusters == 0 && !r.label && !r.off && !r.seq && !r.depth);
    pfl_consensus_free(&r);                                                        /* (an emptied result and NULL are fine) */
    pfl_consensus_free(NULL);
    memset(&r, 0, sizeof r);
    CHECK(pfl_write_flank_fasta(path, "left", &r) == PWR_OK);                      /* no cluster: an empty file */
    remove(path);
    return 0;
}

/* pfl_consensus_pack from sources of exactly their lengths, then through the writer */
static int pack_case(const char *path)
{
    char *s0 = malloc(5), *s2 = malloc(1);
    int *d0 = malloc(sizeof(int) * 5), *d2 = malloc(sizeof(int));
    CHECK(s0 && s2 && d0 && d2);
    memcpy(s0, "aacgt", 5); s2[0] = 'c';
    for (int k = 0; k < 5; k++) d0[k] = 7 - k;
    d2[0] = 2;
    const int label[3] = {0, 4, 11}, members[3] = {7, 0, 2}, backbone[3] = {3, -1, 9}, len[3] = {5, 0, 1};
    const char *seq[3] = {s0, NULL, s2};
    const int *depth[3] = {d0, NULL, d2};
    pfl_consensus_result r;
    CHECK(pfl_consensus_pack(3, label, members, backbone, seq, depth, len, &r) == PWR_OK);
    CHECK(r.nclusters == 3 && r.off[0] == 0 && r.off[1] == 5 && r.off[2] == 5 && r.off[3] == 6 && memcmp(r.seq, "aacgtc", 7) == 0);
    CHECK(r.depth[0] == 7 && r.depth[4] == 3 && r.depth[5] == 2 && r.label[2] == 11 && r.members[1] == 0 && r.backbone[1] == -1);
    CHECK(pfl_write_flank_fasta(path, "left", &r) == PWR_OK);
    pfl_consensus_free(&r);
    remove(path);
    CHECK(pfl_consensus_pack(0, NULL, NULL, NULL, NULL, NULL, NULL, &r) == PWR_OK && r.nclusters == 0 && r.off && r.off[0] == 0 && r.seq[0] == 0);
    pfl_consensus_free(&r);
    const int bad[3] = {5, -1, 1};
    CHECK(pfl_consensus_pack(3, label, members, backbone, seq, depth, bad, &r) == PWR_ERR_ARG && !r.label && !r.off);
    const int need[3] = {5, 2, 1};                                                 /* a length without a sequence */
    CHECK(pfl_consensus_pack(3, label, members, backbone, seq, depth, need, &r) == PWR_ERR_ARG && !r.seq);
    CHECK(pfl_consensus_pack(-1, label, members, backbone, seq, depth, len, &r) == PWR_ERR_ARG);
    CHECK(pfl_consensus_pack(3, label, members, backbone, seq, depth, len, NULL) == PWR_ERR_ARG);
    CHECK(pfl_consensus_pack(3, NULL, members, backbone, seq, depth, len, &r) == PWR_ERR_ARG && !r.label);
    free(s0); free(s2); free(d0); free(d2);
    return 0;
}

int main(int argc, char **argv)
{
    /* a gap emits nothing, an insertion follows its position (a gap's too), the depth is the position's, min_depth cuts */
    static const unsigned char sym[6] = {0, 4, 3, 4, 1, 2}, ins[6] = {0, 2, 0, 0, 4, 1};
    static const int voters[6] = {5, 5, 4, 4, 3, 1};
    static const int d1[7] = {5, 5, 4, 3, 3, 1, 1}, d4[3] = {5, 5, 4};
    if (call_case(6, sym, ins, voters, 1, "actctga", d1) || call_case(6, sym, ins, voters, 2, "actct", d1) ||
        call_case(6, sym, ins, voters, 4, "act", d4) || call_case(6, sym, ins, voters, 6, "", d4) || call_case(0, sym, ins, voters, 1, "", d4))
        return 1;
    /* every position a base and an insertion: the 2 * npos bound is met exactly */
    static unsigned char all_sym[64], all_ins[64];
    static int all_voters[64];
    for (int i = 0; i < 64; i++) { all_sym[i] = (unsigned char)(i & 3); all_ins[i] = (unsigned char)(1 + ((i >> 2) & 3)); all_voters[i] = 9; }
    if (call_case(64, all_sym, all_ins, all_voters, 9, NULL, NULL)) return 1;
    unsigned int state = 2463534242u;
    for (int round = 0; round < 200; round++) {
        static unsigned char rs[300], ri[300];
        static int rv[300];
        state = state * 1664525u + 1013904223u;
        const int npos = (int)((state >> 8) % 301);
        for (int i = 0; i < npos; i++) {
            state = state * 1664525u + 1013904223u;
            rs[i] = (unsigned char)((state >> 8) % 5); ri[i] = (unsigned char)((state >> 12) % 5); rv[i] = (int)((state >> 16) % 12);
        }
        if (call_case(npos, rs, ri, rv, 1 + round % 4, NULL, NULL)) return 1;
    }
    if (fasta_case(argc > 1 ? argv[1] : "flank_consensus_sanitize.fasta")) return 1;
    if (pack_case(argc > 1 ? argv[1] : "flank_consensus_sanitize.fasta")) return 1;
    printf("pfl_call, pfl_consensus_pack, pfl_write_flank_fasta, pfl_consensus_free: all cases hold\n");
    return 0;
}
