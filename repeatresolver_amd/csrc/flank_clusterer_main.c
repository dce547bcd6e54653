/* FlankClusterer: the flank labellings of a repeat from the files the pipeline's front leaves behind (include/pfl.h).  The
 * reference has no such tool: SimDataAssessment.py takes FlankingLeft and FlankingRight from the simulator's ground truth
 * (SDA:226-245).
 *   FlankClusterer Seq.fasta ReadSeqInfo SeqClass -e max_permille [-b strandfile] [-l reach] [-m min_len] [-s min_size]
 *                  [-o prefix] [-g device] [-c extent [-k block] [-d min_depth] [-n rounds]]
 * writes <prefix>_FlankingLeft and <prefix>_FlankingRight, one label per MSA row (-1: no flank, a short one, or a cluster
 * below min_size), as SDA:248-256 would.  The default prefix is Seq.fasta's path before "Seq.fasta", or "Flanks".  With -c
 * it also writes <prefix>_FlankLeft.fasta and <prefix>_FlankRight.fasta: the consensus sequence of every cluster's flanks
 * over at most extent bases from the boundary, in template orientation.  Without -c it does what it did. */
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
    printf("-c <extent> also writes _FlankLeft.fasta and _FlankRight.fasta: every cluster's consensus over extent bases.\n");
    printf("-k <256>   bases of a block of the consensus' alignments, a multiple of 32 up to %d.\n", PFL_MAX_REACH);
    printf("-d <1>     the consensus ends where fewer flanks than this reach.\n");
    printf("-n <2>     rounds: the consensus of a round is the backbone of the next.\n");
    return code;
}

int main(int argc, char **argv)
{
    if (argc < 4) return usage(argc < 2 ? 0 : 1);
    const char *seq = argv[1], *info = argv[2], *cls = argv[3], *strand = NULL, *prefix = NULL;
    int permille = -1, reach = 256, min_len = 100, min_size = 1, device = 0, extent = 0, block = 256, min_depth = 1, rounds = 2;
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
        if (argv[i][1] == 'c' && has) extent = atoi(argv[i + 1]);
        if (argv[i][1] == 'k' && has) block = atoi(argv[i + 1]);
        if (argv[i][1] == 'd' && has) min_depth = atoi(argv[i + 1]);
        if (argv[i][1] == 'n' && has) rounds = atoi(argv[i + 1]);
    }
    if (permille < 0) { printf("FlankClusterer: -e max_permille is required: it has no default.\n"); return 1; }
    if (extent < 0) { printf("FlankClusterer: -c takes the number of bases.\n"); return 1; }
    const size_t sl = strlen(seq), tl = strlen("Seq.fasta");
    size_t pl = prefix ? strlen(prefix) : (sl >= tl && strcmp(seq + sl - tl, "Seq.fasta") == 0) ? sl - tl : 0;
    if (!prefix && pl && seq[pl - 1] == '_') pl--;                                  /* ds_Seq.fasta -> ds_FlankingLeft */
    if (!prefix) prefix = pl ? seq : "Flanks";
    const size_t room = (pl ? pl : strlen(prefix)) + 24;
    char *left = malloc(room), *right = malloc(room), *lfa = malloc(room), *rfa = malloc(room);
    if (!left || !right || !lfa || !rfa) return 1;
    snprintf(lfa, room, "%.*s_FlankLeft.fasta", (int)(pl ? pl : strlen(prefix)), prefix);
    snprintf(rfa, room, "%.*s_FlankRight.fasta", (int)(pl ? pl : strlen(prefix)), prefix);
    snprintf(left, room, "%.*s_FlankingLeft", (int)(pl ? pl : strlen(prefix)), prefix);
    snprintf(right, room, "%.*s_FlankingRight", (int)(pl ? pl : strlen(prefix)), prefix);
    fflush(stdout);
    const int rc = pfl_run_files_consensus(seq, info, cls, strand, permille, reach, min_len, min_size, left, right, extent, block,
                                           min_depth, rounds, lfa, rfa, device, stdout);
    free(left); free(right); free(lfa); free(rfa);
    return rc;
}
