/* LocusAnchorer: where in an assembly the copies of a resolved repeat belong (include/pla.h).  The reference has no such tool.
 *   LocusAnchorer <loci.fasta> <assembly.fasta> -e max_permille -s max_span [-r reach] [-m min_len] [-o prefix] [-g device]
 * loci.fasta is what resolution.write_loci writes: left flank + copy + right flank per whole copy.  The `reach` bases of every
 * flank nearest to the repeat are searched in every contig, in both orientations (the GPU part), and the tool writes
 *   <prefix>_Anchors        one line per hit: locus, side, orientation, contig, boundary, lo, hi, distance
 *   <prefix>_Placements     one line per locus: its status and where it lies
 *   <prefix>_Patched.fasta  the assembly with every PLACED interval replaced by the locus's copy
 * The default prefix is "Anchors". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pla.h"

static int usage(int code)
{
    printf("Usage: ./LocusAnchorer loci.fasta assembly.fasta -e max_permille -s max_span\n");
    printf("Flags:\n");
    printf("-e         a flank is found where its edit distance is at most e/1000 of the searched bases (0 .. 500).\n");
    printf("-s         the most bases of the assembly that may lie between a locus's two boundaries.\n");
    printf("-r <256>   how many bases of a flank from the repeat boundary are searched, up to %d.\n", PLA_MAX_REACH);
    printf("-m <100>   flanks shorter than this are not searched.\n");
    printf("-o <prefix> of _Anchors, _Placements and _Patched.fasta.\n");
    printf("-g <0>     device.\n");
    return code;
}

int main(int argc, char **argv)
{
    if (argc < 3) return usage(argc < 2 ? 0 : 1);
    const char *prefix = "Anchors";
    int permille = -1, span = -1, reach = 256, min_len = 100, device = 0;
    for (int i = 3; i < argc; i++) {
        if (argv[i][0] != '-') continue;
        const int has = i + 1 < argc;
        if (argv[i][1] == 'h') return usage(0);
        if (argv[i][1] == 'e' && has) permille = atoi(argv[i + 1]);
        if (argv[i][1] == 's' && has) span = atoi(argv[i + 1]);
        if (argv[i][1] == 'r' && has) reach = atoi(argv[i + 1]);
        if (argv[i][1] == 'm' && has) min_len = atoi(argv[i + 1]);
        if (argv[i][1] == 'o' && has) prefix = argv[i + 1];
        if (argv[i][1] == 'g' && has) device = atoi(argv[i + 1]);
    }
    if (permille < 0) { printf("LocusAnchorer: -e max_permille is required: it has no default.\n"); return 1; }
    if (span < 0) { printf("LocusAnchorer: -s max_span is required: it has no default.\n"); return 1; }
    fflush(stdout);
    return pla_run_files(argv[1], argv[2], permille, span, reach, min_len, prefix, device, stdout);
}
