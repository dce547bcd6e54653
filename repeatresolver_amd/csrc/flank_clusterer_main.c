/* FlankClusterer: the flank labellings of a repeat from the files the pipeline's front leaves behind (include/pfl.h).  The
 * reference has no such tool: SimDataAssessment.py takes FlankingLeft and FlankingRight from the simulator's ground truth
 * (SDA:226-245).
 *   FlankClusterer Seq.fasta ReadSeqInfo SeqClass -e max_permille [-b strandfile] [-l reach] [-m min_len] [-s min_size]
 *                  [-o prefix] [-g device]
 * writes <prefix>_FlankingLeft and <prefix>_FlankingRight, one label per MSA row (-1: no flank, a short one, or a cluster
 * below min_size), as SDA:248-256 would.  The default prefix is Seq.fasta's path before "Seq.fasta", or "Flanks". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfl.h"

static int usage(int code)
{
    printf("Usage: ./FlankClusterer Seq.fasta ReadSeqInfo SeqClass -e max_permille\n");
    printf("Flags:\n");
    printf("-e         joins two flanks whose anchored edit distance is at most e/1000 of the shorter one's compared bases.\n");
    printf("-b <file>  InitialAligner's strand file (-b there): the rows marked - are reverse complements.\n");
    printf("-l <256>   how many bases from the repeat boundary are compared.\n");
    printf("-m <100>   flanks shorter than this get no label.\n");
    printf("-s <1>     clusters smaller than this get no label.\n");
    printf("-o <prefix> of _FlankingLeft and _FlankingRight.\n");
    return code;
}

int main(int argc, char **argv)
{
    if (argc < 4) return usage(argc < 2 ? 0 : 1);
    const char *seq = argv[1], *info = argv[2], *cls = argv[3], *strand = NULL, *prefix = NULL;
    int permille = -1, reach = 256, min_len = 100, min_size = 1, device = 0;
    for (int i = 4; i < argc; i++) {
        if (argv[i][0] != '-') continue;
        const int has = i + 1 < argc;
        if (argv[i][1] == 'h') return usage(0);
        if (argv[i][1] == 'e' && has) permille = atoi(argv[i + 1]);
        if (argv[i][1] == 'b' && has) strand = argv[i + 1];
        if (argv[i][1] == 'l' && has) reach = atoi(argv[i + 1]);
        if (argv[i][1] == 'm' && has) min_len = atoi(argv[i + 1]);
        if (argv[i][1] == 's' && has) min_size = atoi(argv[i + 1]);
        if (argv[i][1] == 'o' && has) prefix = argv[i + 1];
        if (argv[i][1] == 'g' && has) device = atoi(argv[i + 1]);
    }
    if (permille < 0) { printf("FlankClusterer: -e max_permille is required: it has no default.\n"); return 1; }
    const size_t sl = strlen(seq), tl = strlen("Seq.fasta");
    size_t pl = prefix ? strlen(prefix) : (sl >= tl && strcmp(seq + sl - tl, "Seq.fasta") == 0) ? sl - tl : 0;
    if (!prefix && pl && seq[pl - 1] == '_') pl--;                                  /* ds_Seq.fasta -> ds_FlankingLeft */
    if (!prefix) prefix = pl ? seq : "Flanks";
    const size_t room = (pl ? pl : strlen(prefix)) + 20;
    char *left = malloc(room), *right = malloc(room);
    if (!left || !right) return 1;
    snprintf(left, room, "%.*s_FlankingLeft", (int)(pl ? pl : strlen(prefix)), prefix);
    snprintf(right, room, "%.*s_FlankingRight", (int)(pl ? pl : strlen(prefix)), prefix);
    fflush(stdout);
    const int rc = pfl_run_files(seq, info, cls, strand, permille, reach, min_len, min_size, left, right, device, stdout);
    free(left); free(right);
    return rc;
}
