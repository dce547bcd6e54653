// pgr_assign_device.hip -- MI355X (gfx950): every row of a device-resident MSA against the consensus of every part of a
// labelling, behind include/pgr.h (pgr_msa_assign): per (row, part) the compared columns in which the row differs from the
// part's consensus, per row the columns in which it has a symbol, and the best and the second part.
//
// The reference (PhilippBongartz/RepeatResolver) has no counterpart: the semantics are this project's own and stand in the
// header.  Everything is an integer; there are no atomics, so no result depends on an order.  The kernels are shells around
// the bodies of row_planes.h, which pgr_settle_device.hip shares:
//   k_as_planes  the rows of a range as bit planes over the compared columns, planes[word][row of the range] = {valid, bit0,
//                bit1, bit2}: the layout the next kernel streams.
//   k_as_dist    the tiled product in the manner of four_count_tile.h, with the tile in scalar registers instead of LDS.  A
//                work-group has 64 rows (one per lane) and a tile of PGR_AS_TILE parts; its RP_NW waves share the words: a
//                range of rows at the benchmark's size is about a thousand rows, and rows x part tiles alone would leave most
//                of the chip idle.  (Staged in LDS, every (row, part, word) would read three 64-bit words by broadcast: as
//                many LDS cycles as its twelve vector instructions take on the four SIMDs that share one LDS.)  Every compared
//                column counts for every row: no mask.  mismatches[row][part], compared[row].
//   k_as_best    a thread per row over the finished matrix: the fewest mismatches, the lowest index among equals; the same
//                over the other parts.
// The part planes (no valid plane: every compared column counts for every part) are built on the host and uploaded, padded
// with zeros to whole tiles.
// A range of rows holds 32 bytes per row and word of planes and 4 bytes per row and part of the matrix: ranges of at most
// PGR_AS_SCRATCH_BYTES, halved while the device refuses.  Every index into the text is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <vector>

#define PWR_STAGE "pgr"
#include "dev_util.h"
#include "pgr.h"
#include "pgr_internal.h"
#include "row_planes.h"

static double g_as_ms[5] = {0, 0, 0, 0, 0};

// grid (words, groups of 4 x 64 rows), 256 threads.  The range is the rows [r_lo, r_lo + R) of the text.
__global__ __launch_bounds__(256) void k_as_planes(long long width, int r_lo, int R, int ncolumns, const unsigned char *__restrict__ text,
                                                   const int *__restrict__ columns, ulonglong4 *__restrict__ planes)
{
    row_planes_group(width, r_lo, R, ncolumns, text, columns, planes);
}

// grid (R / RP_ROWS, tiles of parts), 64 * RP_NW threads; mat[row][parts]
__global__ __launch_bounds__(64 * RP_NW) void k_as_dist(int R, int parts, int ppad, int nw, const ulonglong4 *__restrict__ planes,
                                                        const u64 *__restrict__ pp, int *__restrict__ mat, int *__restrict__ compared)
{
    row_part_distances(R, parts, ppad, parts, nw, planes, pp, nullptr, mat, compared);
}

// a thread per row: the first smallest value of its row of the matrix, and the first smallest among the others
__global__ __launch_bounds__(256) void k_as_best(int R, int parts, const int *__restrict__ mat, const int *__restrict__ compared,
                                                 int *__restrict__ best, int *__restrict__ second, int *__restrict__ best_m, int *__restrict__ second_m)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const BestSecond x = best_and_second(mat + (size_t)r * parts, parts, compared[r]);
    best[r] = x.b; second[r] = x.s;
    best_m[r] = x.b < 0 ? 0 : x.bm; second_m[r] = x.s < 0 ? 0 : x.sm;
}

extern "C" void pgr_assignment_free(pgr_assignment *o)
{
    if (!o) return;
    free(o->compared); free(o->best); free(o->second); free(o->best_mismatches); free(o->second_mismatches); free(o->mismatches);
    memset(o, 0, sizeof *o);
}

extern "C" int pgr_last_assign_timing(double *ms5)
{
    if (!ms5) return PWR_ERR_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = g_as_ms[i];
    return PWR_OK;
}

namespace {
// the device buffers of one range of rows
struct Range {
    ulonglong4 *planes = nullptr;
    int *mat = nullptr, *per_row = nullptr;                            // per_row: compared, best, second and the two counts, R each
    DevArena mem;
    bool get(size_t R, size_t nw, size_t parts)
    {
        planes = mem.get<ulonglong4>(nw * R); mat = mem.get<int>(R * parts); per_row = mem.get<int>(5 * R);
        return planes && mat && per_row;
    }
};
}

static int assign(const pgr_msa *h, int parts, int von, int width, const unsigned char *codes, int ncolumns, const int *columns,
                  int want_matrix, pgr_assignment *o)
{
    const double t0 = now_ms();
    const int rows = h->rows;
    if (parts < 1 || width < 1 || ncolumns < 1 || von < 0 || (long long)von + width > h->width) return PWR_ERR_ARG;
    if (parts > PGR_MAX_ROWS) return PWR_ERR_RANGE;
    for (int j = 0; j < ncolumns; ++j)
        if (columns[j] < von || columns[j] > von + width - 1 || (j > 0 && columns[j] <= columns[j - 1])) return PWR_ERR_ARG;
    unsigned int above = 0;                                            // (no early exit: the loop is vectorised)
    for (size_t i = 0, n = (size_t)parts * width; i < n; ++i) above |= codes[i] > 4;
    if (above) return PWR_ERR_ARG;

    o->rows = rows; o->parts = parts; o->ncolumns = ncolumns;
    int **per_row[5] = {&o->compared, &o->best, &o->second, &o->best_mismatches, &o->second_mismatches};
    for (int **p : per_row)
        if (!(*p = (int *)malloc(sizeof(int) * (rows > 0 ? rows : 1)))) return PWR_ERR_NOMEM;
    if (want_matrix && !(o->mismatches = (int *)malloc(sizeof(int) * (rows > 0 ? (size_t)rows : 1) * parts))) return PWR_ERR_NOMEM;

    // the parts' three bit planes over the compared columns: pp[word][plane][part]
    const int nw = (ncolumns + 63) / 64;
    const int ppad = (parts + RP_TP - 1) / RP_TP * RP_TP;              // whole tiles: the padding stays zero
    std::vector<u64> pp((size_t)nw * 3 * ppad, 0ull);
    for (int p = 0; p < parts; ++p) {
        const unsigned char *c = codes + (size_t)p * width;
        for (int w = 0; w < nw; ++w) {
            u64 b0 = 0, b1 = 0, b2 = 0;
            for (int j = w * 64, e = std::min(ncolumns, j + 64), i = 0; j < e; ++j, ++i) {
                const u64 x = c[columns[j] - von];
                b0 |= (x & 1) << i; b1 |= ((x >> 1) & 1) << i; b2 |= (x >> 2) << i;
            }
            u64 *at = &pp[(size_t)w * 3 * ppad + p];
            at[0] = b0; at[ppad] = b1; at[2 * (size_t)ppad] = b2;
        }
    }

    if (hipSetDevice(h->device) != hipSuccess) return PWR_ERR_DEVICE;
    DevArena mem;
    int *d_columns = mem.put(columns, (size_t)ncolumns);
    u64 *d_pp = mem.put(pp.data(), pp.size());
    if (!d_columns || !d_pp) return mem.err;

    // the longest range of rows whose planes and matrix stay within PGR_AS_SCRATCH_BYTES (one row at least) and fit the device
    const long long per = (long long)PGR_AS_SCRATCH_BYTES / (32LL * nw + 4LL * parts);
    int R = (int)std::max(1LL, std::min((long long)rows, per));
    std::optional<Range> rg;
    if (const int rc = largest_that_fits(R, [&](int n) { return rg.emplace().get((size_t)n, (size_t)nw, (size_t)parts); })) return rc;
    HIPC(hipDeviceSynchronize());
    double t = now_ms(), u;
    g_as_ms[1] = t - t0; g_as_ms[2] = g_as_ms[3] = g_as_ms[4] = 0;

    for (int r_lo = 0; r_lo < rows; r_lo += R) {
        const int n = std::min(R, rows - r_lo);                        // rows of this range; the buffers are laid out for n, not R
        int *d_cmp = rg->per_row, *d_best = d_cmp + n, *d_second = d_best + n, *d_bm = d_second + n, *d_sm = d_bm + n;
        hipLaunchKernelGGL(k_as_planes, dim3(nw, (n + 255) / 256), dim3(256), 0, 0, (long long)h->width, r_lo, n, ncolumns,
                           (const unsigned char *)h->text, d_columns, rg->planes);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_as_ms[2] += u - t; t = u;
        hipLaunchKernelGGL(k_as_dist, dim3((n + RP_ROWS - 1) / RP_ROWS, ppad / RP_TP), dim3(64 * RP_NW), 0, 0, n, parts, ppad, nw,
                           (const ulonglong4 *)rg->planes, (const u64 *)d_pp, rg->mat, d_cmp);
        HIPC(hipGetLastError());
        hipLaunchKernelGGL(k_as_best, dim3((n + 255) / 256), dim3(256), 0, 0, n, parts, (const int *)rg->mat, (const int *)d_cmp, d_best,
                           d_second, d_bm, d_sm);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_as_ms[3] += u - t; t = u;
        int *const from[5] = {d_cmp, d_best, d_second, d_bm, d_sm};
        for (int i = 0; i < 5; ++i) HIPC(hipMemcpy(*per_row[i] + r_lo, from[i], sizeof(int) * n, hipMemcpyDeviceToHost));
        if (want_matrix) HIPC(hipMemcpy(o->mismatches + (size_t)r_lo * parts, rg->mat, sizeof(int) * (size_t)n * parts, hipMemcpyDeviceToHost));
        u = now_ms(); g_as_ms[4] += u - t; t = u;
    }
    g_as_ms[0] = t - t0;
    return PWR_OK;
}

extern "C" int pgr_msa_assign(pgr_msa *h, int parts, int von, int width, const unsigned char *codes, int ncolumns, const int *columns,
                              int want_matrix, pgr_assignment *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!h || !codes || !columns) return PWR_ERR_ARG;
    const int rc = abi_guard([&] { return assign(h, parts, von, width, codes, ncolumns, columns, want_matrix, out); });
    if (rc) pgr_assignment_free(out);
    return rc;
}
