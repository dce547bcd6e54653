/* Drop-in for the reference's `ReadCutter` (ReadCutter.c main(), RC:939-1112): same argv, same files, same stdout including the
 * progress lines; the edit-distance rows run on the GPU behind include/prc.h.  Extra flags: -g <device>, -b 1: reads may lie
 * on either strand (prc_cut_strands); without it nothing changes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "prc.h"

static void help(void)
{
    printf("Usage: ./ReadCutter template.fasta reads.fasta\n");                                                        /* RC:876-881 */
    printf("Flags:\n");
    printf("-p <20>    determines the number of parts into which the template is cut and which are mapped into the reads.\n");
    printf("-e <0.30>  is the mapping error cutoff being used to detect occurences of parts in reads\n");
    printf("-w <150>   restricts how far apart and close together mappings can be.\n");
    printf("-l <0>     is used to create parts which overlap by l bases.\n");
    printf("-b <0>     1: reads may lie on either strand; the parts are also mapped into each read's reverse complement.\n");
    exit(0);
}

int main(int argc, char **argv)
{
    if (argc < 3) { printf("Usage: ./ReadCutter template.fasta Reads.fasta\n"); return argc < 2 ? 0 : 1; }          /* RC:944 */
    const char *templ_path = argv[1], *reads_path = argv[2];
    /* default outputs: the template path's prefix before "Template.fasta" + "Seq.fasta" / "ReadSeqInfo" (RC:953-970),
     * printed before the flags are read (RC:972-973) */
    const size_t tl = strlen(templ_path), sl = strlen("Template.fasta");
    const size_t pl = (tl >= sl && strcmp(templ_path + tl - sl, "Template.fasta") == 0) ? tl - sl : 0;
    char *out_seq = malloc(pl + 16), *out_info = malloc(pl + 16);
    if (!out_seq || !out_info) return 1;
    snprintf(out_seq, pl + 16, "%.*sSeq.fasta", (int)pl, templ_path);
    snprintf(out_info, pl + 16, "%.*sReadSeqInfo", (int)pl, templ_path);
    printf("outputfile: %s\n", out_seq);
    printf("readseqfile: %s\n", out_info);
    const char *seq = out_seq, *info = out_info;
    int parts = 60, overlap = 0, wiggleroom = 150, device = 0, both_strands = 0;
    double error_cutoff = 0.30;
    for (int i = 1; i < argc; i++) {                                                                                   /* RC:991-1030 */
        if (argv[i][0] != '-') continue;
        const int has = i + 1 < argc;                  /* (the reference reads argv[argc] == NULL for a value-less last flag) */
        if (argv[i][1] == 'o' && has) seq = argv[i + 1];
        if (argv[i][1] == 'r' && has) info = argv[i + 1];
        if (argv[i][1] == 'p' && has) parts = atoi(argv[i + 1]);
        if (argv[i][1] == 'l' && has) overlap = atoi(argv[i + 1]);
        if (argv[i][1] == 'w' && has) wiggleroom = atoi(argv[i + 1]);
        if (argv[i][1] == 'e' && has) error_cutoff = atof(argv[i + 1]);
        if (argv[i][1] == 'g' && has) device = atoi(argv[i + 1]);
        if (argv[i][1] == 'b' && has) both_strands = atoi(argv[i + 1]) != 0;
        if (argv[i][1] == 'h') help();
    }
    fflush(stdout);
    const int rc = prc_run_files_strands(templ_path, reads_path, seq, info, parts, overlap, error_cutoff, wiggleroom, both_strands,
                                         device, stdout);
    free(out_seq); free(out_info);
    return rc;
}
