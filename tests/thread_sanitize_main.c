/* TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  pgr_thread (repeatresolver_amd/csrc/pgr_host.c) under the host sanitizers, as a program
 * of its own: the labellings of tests/cx_cases.py (THREAD_CASES, the same numbers) and random ones of 300 rows in 5 labellings,
 * the refusals, and the invariants of the header checked on every result.  From the repository's root:
 *   cc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irepeatresolver_amd/csrc \
 *      tests/thread_sanitize_main.c repeatresolver_amd/csrc/pgr_host.c -lm -o thread_sanitize && ./thread_sanitize
 * It prints one line and returns 0 when every check holds; a sanitizer report ends it with a non-zero status. */
#include <stdio.h>
#include <stdlib.h>

#include "pgr.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static int run(int nres, int rows, const int *labels, int want_threads)
{
    pgr_threads t;
    CHECK(pgr_thread(nres, rows, labels, &t) == PWR_OK);
    CHECK(t.nres == nres && t.rows == rows && t.nthreads >= 1 && t.offset[0] == 0);
    CHECK(want_threads < 0 || t.nthreads == want_threads);
    int *members = calloc((size_t)t.nthreads, sizeof(int));
    CHECK(members);
    for (int i = 0; i < nres; i++)
        for (int l = 0; l < t.offset[i + 1] - t.offset[i]; l++) {
            int occurs = 0;
            for (int r = 0; r < rows; r++) occurs |= labels[(size_t)i * rows + r] == l;
            const int th = t.thread_of[t.offset[i] + l];
            CHECK(occurs ? th >= 0 && th < t.nthreads : th == -1);
            if (occurs) { CHECK(t.first[th] <= i && i <= t.last[th]); members[th]++; }
        }
    for (int th = 0; th < t.nthreads; th++) CHECK(members[th] == t.last[th] - t.first[th] + 1);   /* one label per labelling, no hole */
    free(members);
    for (int r = 0; r < rows; r++) {
        int seen = -1, conflict = 0;
        for (int i = 0; i < nres; i++) {
            const int l = labels[(size_t)i * rows + r];
            if (l < 0) continue;
            const int th = t.thread_of[t.offset[i] + l];
            if (seen < 0) seen = th; else if (seen != th) conflict = 1;
        }
        CHECK(t.row_conflict[r] == conflict && t.row_thread[r] == (conflict ? -1 : seen));
    }
    pgr_threads_free(&t);
    CHECK(t.nthreads == 0 && !t.first && !t.thread_of);
    return 0;
}

int main(void)
{
    static const int identical[3][7] = {{0, 0, 1, 1, 2, 2, -1}, {0, 0, 1, 1, 2, 2, -1}, {0, 0, 1, 1, 2, 2, -1}};
    static const int split[2][8] = {{0, 0, 0, 0, 0, 1, 1, 1}, {0, 0, 0, 1, 1, 2, 2, 2}};
    static const int vanish[3][6] = {{0, 0, 0, 1, 1, 1}, {0, 0, 0, -1, -1, -1}, {0, 0, 0, 1, 1, 1}};
    static const int ties[2][9] = {{0, 0, 0, 0, 0, 0, 1, 1, 2}, {0, 0, 1, 1, 2, 2, 2, 2, 3}};
    static const int minus[3][7] = {{0, -1, 0, 1, -1, 3, 3}, {0, 0, -1, 1, -1, 2, 2}, {-1, 0, 0, 1, -1, 2, -1}};
    static const int conflict[2][7] = {{0, 0, 0, 1, 1, 1, 0}, {0, 0, 0, 1, 1, 1, 1}};
    if (run(3, 7, &identical[0][0], 3) || run(2, 8, &split[0][0], 3) || run(3, 6, &vanish[0][0], 3) || run(2, 9, &ties[0][0], 5) ||
        run(3, 7, &minus[0][0], -1) || run(2, 7, &conflict[0][0], 2))
        return 1;
    /* 300 rows in 5 labellings: six copies, labels permuted per labelling, a tenth of the rows left out, a tenth at random */
    static int random_labels[5][300];
    unsigned int state = 12345u;
    for (int round = 0; round < 20; round++) {
        for (int i = 0; i < 5; i++)
            for (int r = 0; r < 300; r++) {
                state = state * 1664525u + 1013904223u;
                const unsigned int x = state >> 8, kind = x % 10;
                random_labels[i][r] = kind == 0 ? -1 : kind == 1 ? (int)((x >> 4) % 7) : (r % 6 + i + round) % 7;
            }
        if (run(5, 300, &random_labels[0][0], -1)) return 1;
    }
    /* a single label value far from the others: large, sparse matrices */
    static int sparse[2][4] = {{0, 2999, 0, -1}, {1500, 0, 1500, 7}};
    if (run(2, 4, &sparse[0][0], -1)) return 1;
    /* the refusals leave *out empty */
    pgr_threads t;
    static const int below[2][3] = {{0, 1, -2}, {1, 0, 0}}, none[2][3] = {{0, 1, 1}, {-1, -1, -1}};
    CHECK(pgr_thread(2, 3, &below[0][0], NULL) == PWR_ERR_ARG);
    CHECK(pgr_thread(2, 3, NULL, &t) == PWR_ERR_ARG && !t.first);
    CHECK(pgr_thread(1, 3, &below[0][0], &t) == PWR_ERR_ARG && pgr_thread(2, 0, &below[0][0], &t) == PWR_ERR_ARG);
    CHECK(pgr_thread(2, 3, &below[0][0], &t) == PWR_ERR_ARG && !t.first && !t.offset && !t.thread_of && t.nres == 0);
    CHECK(pgr_thread(2, 3, &none[0][0], &t) == PWR_ERR_ARG && !t.first && !t.offset);
    pgr_threads_free(NULL);
    printf("pgr_thread: all labellings and refusals hold\n");
    return 0;
}
