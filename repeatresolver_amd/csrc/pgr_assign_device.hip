// pgr_assign_device.hip -- MI355X (gfx950): every row of a device-resident MSA against the consensus of every part of a
// labelling, behind include/pgr.h (pgr_msa_assign): per (row, part) the compared columns in which the row differs from the
// part's consensus, per row the columns in which it has a symbol, and the best and the second part.
//
// The reference (PhilippBongartz/RepeatResolver) has no counterpart: the semantics are this project's own and stand in the
// header.  Everything is an integer; there are no atomics, so no result depends on an order.
//   k_as_planes  the rows of a range as bit planes over the compared columns.  A wave owns 64 entries of columns[] (one word)
//                and a group of 64 rows, which it reads one after the other: a lane loads its byte of the row, one compare per
//                symbol of base_code.h is a __ballot, the row's words of the planes valid, bit0, bit1, bit2 are ORs of those
//                masks, and lane i keeps those of the group's i-th row.  After the group the wave stores 64 neighbouring rows of each
//                plane at once: planes[word][plane][row of the range], the layout the next kernel streams.
//   k_as_dist    the tiled product in the manner of four_count_tile.h, with the tile in scalar registers instead of LDS.  A
//                work-group has 64 rows (one per lane) and a tile of PGR_AS_TILE parts; its AS_NW waves share the words (wave s
//                takes the words w = s mod AS_NW): a range of rows at the benchmark's size is about a thousand rows, and rows
//                x part tiles alone would leave most of the chip idle.  The address of a part's plane word does not depend on
//                the lane, so the tile's 3 x PGR_AS_TILE words of a word index come by scalar loads and are operands of the
//                vector instructions as they are: no LDS traffic, no barrier inside the loop.  (Staged in LDS, every
//                (row, part, word) would read three 64-bit words by broadcast: as many LDS cycles as its twelve vector
//                instructions take on the four SIMDs that share one LDS.)  Per (row, part, word)
//                d = ((r0 ^ p0) | (r1 ^ p1) | (r2 ^ p2)) & valid, m += popcount(d).  The counters stay in registers; at the
//                end every wave puts its counters into LDS and wave j adds up counter j of all waves and stores
//                mismatches[row][part], or, for the last counter in the first tile of parts, compared[row] = the popcount
//                of valid.  The part planes are padded with zeros to whole tiles on the host, so that no load of a tile needs
//                a condition; a slot without a part stores nothing.
//   k_as_best    a thread per row over the finished matrix: the fewest mismatches, the lowest index among equals; the same
//                over the other parts.
// The part planes (no valid plane: every compared column counts for every part) are built on the host and uploaded.
// A range of rows holds 32 bytes per row and word of planes and 4 bytes per row and part of the matrix: ranges of at most
// PGR_AS_SCRATCH_BYTES, halved while the device refuses.  Every index into the text is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <vector>

#define PWR_STAGE "pgr"
#include "dev_util.h"
#include "pgr.h"
#include "pgr_internal.h"

#define AS_TP PGR_AS_TILE        // parts per tile
#define AS_NW 16                 // waves of a work-group of k_as_dist: they share the words
#define AS_ROWS 64               // rows per work-group of k_as_dist: one per lane
static_assert(AS_TP == 8, "3 x 8 plane words of a tile are 48 scalar registers; eight counters per thread");

typedef unsigned long long u64;

static double g_as_ms[5] = {0, 0, 0, 0, 0};

// grid (words, groups of 4 x 64 rows), 256 threads.  The range is the rows [r_lo, r_lo + R) of the text.
__global__ __launch_bounds__(256) void k_as_planes(long long width, int r_lo, int R, int ncolumns, const unsigned char *__restrict__ text,
                                                   const int *__restrict__ columns, u64 *__restrict__ planes)
{
    const int lane = threadIdx.x & 63, row0 = (blockIdx.y * 4 + (int)(threadIdx.x >> 6)) * 64;
    if (row0 >= R) return;                                             // (the same for the whole wave)
    const int w = blockIdx.x, j = w * 64 + lane, n = min(64, R - row0);
    const bool in = j < ncolumns;                                      // a lane behind the last column loads nothing and is valid nowhere
    const unsigned char *p = text + (long long)(r_lo + row0) * width + (in ? columns[j] : 0);
    u64 keep[4] = {0, 0, 0, 0};
    for (int i0 = 0; i0 < n; i0 += 8) {
        unsigned int ch[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)                                    // eight loads in flight; behind the group's last row that row again, kept by no lane
            ch[i] = in ? p[(long long)min(i0 + i, n - 1) * width] : ' ';
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // base_code.h as one compare per symbol, whose result is the ballot already: a letter in lower case (no other byte
            // becomes one of a c g t), the two gaps as they are.  The codes' bits are sums of these masks, on the scalar unit.
            const unsigned int f = ch[i] | 0x20u;
            const u64 c = __ballot(f == 'c'), g = __ballot(f == 'g'), t = __ballot(f == 't');
            const u64 gap = __ballot(ch[i] == '-') | __ballot(ch[i] == '_'), v = __ballot(f == 'a') | c | g | t | gap;
            if (lane == i0 + i) { keep[0] = v; keep[1] = c | t; keep[2] = g | t; keep[3] = gap; }
        }
    }
    if (lane < n)
#pragma unroll
        for (int k = 0; k < 4; ++k) planes[((size_t)w * 4 + k) * R + row0 + lane] = keep[k];
}

// grid (R / AS_ROWS, tiles of parts), 64 * AS_NW threads: lane = the row, wave = the words.  pp[word][plane 0..2][ppad], ppad =
// the parts rounded up to whole tiles, the padding zero.
__global__ __launch_bounds__(64 * AS_NW) void k_as_dist(int R, int parts, int ppad, int nw, const u64 *__restrict__ planes,
                                                        const u64 *__restrict__ pp, int *__restrict__ mat, int *__restrict__ compared)
{
    __shared__ int red[AS_NW][AS_TP + 1][64];                          // every wave's counters, the last one compared
    const int lane = threadIdx.x & 63, p0 = blockIdx.y * AS_TP, row = blockIdx.x * AS_ROWS + lane;
    const int slice = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // the same for the wave, and known to be: what follows from it is scalar
    const bool has = row < R;
    int m[AS_TP], cmp = 0;
#pragma unroll
    for (int a = 0; a < AS_TP; ++a) m[a] = 0;
    for (int w = slice; w < nw; w += AS_NW) {
        const u64 *r = planes + (size_t)w * 4 * R + row;               // a thread without a row loads nothing
        const u64 rv = has ? r[0] : 0ull, r0 = has ? r[R] : 0ull, r1 = has ? r[2 * (size_t)R] : 0ull, r2 = has ? r[3 * (size_t)R] : 0ull;
        const u64 *q = pp + (size_t)w * 3 * ppad + p0;                 // (the same address in every lane: scalar loads)
        cmp += __popcll(rv);
#pragma unroll
        for (int a = 0; a < AS_TP; ++a) m[a] += __popcll(((r0 ^ q[a]) | (r1 ^ q[ppad + a]) | (r2 ^ q[2 * (size_t)ppad + a])) & rv);
    }
#pragma unroll
    for (int a = 0; a < AS_TP; ++a) red[slice][a][lane] = m[a];
    red[slice][AS_TP][lane] = cmp;
    __syncthreads();
    for (int j = slice; j <= AS_TP; j += AS_NW) {                      // counter j of all waves, by wave j
        int sum = 0;
#pragma unroll
        for (int o = 0; o < AS_NW; ++o) sum += red[o][j][lane];
        if (!has) continue;
        if (j == AS_TP) { if (blockIdx.y == 0) compared[row] = sum; }
        else if (p0 + j < parts) mat[(size_t)row * parts + p0 + j] = sum;
    }
}

// a thread per row: the first smallest value of its row of the matrix, and the first smallest among the others
__global__ __launch_bounds__(256) void k_as_best(int R, int parts, const int *__restrict__ mat, const int *__restrict__ compared,
                                                 int *__restrict__ best, int *__restrict__ second, int *__restrict__ best_m, int *__restrict__ second_m)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int b = -1, s = -1, bm = INT_MAX, sm = INT_MAX;
    if (compared[r] > 0) {
        const int *row = mat + (size_t)r * parts;
        for (int p = 0; p < parts; ++p) {
            const int v = row[p];
            // the best that is displaced becomes the second: it is smaller than the second, or equal and of lower index
            if (v < bm) { s = b; sm = bm; b = p; bm = v; }
            else if (v < sm) { s = p; sm = v; }
        }
    }
    best[r] = b; second[r] = s;
    best_m[r] = b < 0 ? 0 : bm; second_m[r] = s < 0 ? 0 : sm;
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
    u64 *planes = nullptr;
    int *mat = nullptr, *per_row = nullptr;                            // per_row: compared, best, second and the two counts, R each
    DevArena mem;
    bool get(size_t R, size_t nw, size_t parts)
    {
        planes = mem.get<u64>(nw * 4 * R); mat = mem.get<int>(R * parts); per_row = mem.get<int>(5 * R);
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
    const int ppad = (parts + AS_TP - 1) / AS_TP * AS_TP;              // whole tiles: the padding stays zero
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
    for (;; R = (R + 1) / 2) {
        rg.emplace();
        if (rg->get((size_t)R, (size_t)nw, (size_t)parts)) break;
        (void)hipGetLastError();
        rg.reset();
        if (R == 1) return PWR_ERR_NOMEM;
    }
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
        hipLaunchKernelGGL(k_as_dist, dim3((n + AS_ROWS - 1) / AS_ROWS, ppad / AS_TP), dim3(64 * AS_NW), 0, 0, n, parts, ppad, nw,
                           (const u64 *)rg->planes, (const u64 *)d_pp, rg->mat, d_cmp);
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
