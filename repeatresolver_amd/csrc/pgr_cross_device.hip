// pgr_cross_device.hip -- MI355X (gfx950): every row of a device-resident MSA against the consensus of every part, segment by
// segment of the compared columns, and per row the best explanation by two different parts joined at a segment boundary (a
// crossover), behind include/pgr.h (pgr_msa_crossovers).
//
// The reference (PhilippBongartz/RepeatResolver) has no counterpart: the semantics are this project's own and stand in the
// header.  Everything is an integer; there are no atomics, so no result depends on an order.
//   k_cx_planes  the plane body of row_planes.h (k_as_planes of pgr_assign_device.hip) over the PADDED column list: the host
//                repeats the last column of every segment until the segment ends on a word of 64 entries, so that a word belongs
//                to one segment; mask[word] clears the padding.  planes[word][row of the range] = {valid, bit0, bit1, bit2}.
//   k_cx_dist    the XOR-and-popcount core of row_part_distances (row_planes.h): a lane per row, a tile of PGR_AS_TILE parts
//                whose plane words come by scalar loads.  A wave owns one (group of 64 rows, part tile, segment) and runs over
//                that segment's words only: no LDS, no barrier; the counters go from registers to mm[row][segment][part], the
//                popcount of the valid word, for the first tile, to seg_compared[row][segment].
//   k_cx_cross   a wave per row, lanes over the parts (part p belongs to lane p mod 64: a lane only ever reads what it has
//                written itself).  First pass: per segment the first smallest count (seg_best), and mm turned into prefix sums
//                over the segments in place: L[k][a] = pre[k - 1][a], R[k][b] = pre[nseg - 1][b] - pre[k - 1][b].  Then per
//                admissible split k the first smallest and the first smallest among the others of R[k][.] by a wave
//                reduction; lane a takes b = the first where a differs from it, else the other; a lexicographic (total, a)
//                wave reduction; a later k is kept only when its total is strictly smaller.  That is the (total, k, a, b)
//                order of the header.
//   k_cx_best    a thread per row over the last prefix row, which is the matrix of pgr_msa_assign: best_and_second.
// The padded column list, the masks, the word range of every segment and the parts' planes (over the padded list) are built on
// the host and uploaded.  A range of rows holds 32 bytes per row and word of planes, 4 bytes per row, segment and part of the
// matrix and 8 * nseg + 40 bytes per row of results: ranges of at most PGR_AS_SCRATCH_BYTES, halved while the device refuses.
// Every index into the text and the matrix is 64-bit.
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

#define CX_ROW_INTS 10           // per-row results of a range: the five one-copy fields and the five of the crossover

static double g_cx_ms[6] = {0, 0, 0, 0, 0, 0};

// grid (words, groups of 4 x 64 rows), 256 threads.  The range is the rows [r_lo, r_lo + R) of the text; columns[words * 64]
__global__ __launch_bounds__(256) void k_cx_planes(long long width, int r_lo, int R, int ncolumns, const unsigned char *__restrict__ text,
                                                   const int *__restrict__ columns, ulonglong4 *__restrict__ planes)
{
    row_planes_group(width, r_lo, R, ncolumns, text, columns, planes);
}

// grid (groups of 4 x 64 rows, tiles of parts, segments), 256 threads: a wave per group of 64 rows, lane = the row.  The words
// of segment s are [seg_word[s], seg_word[s + 1]); mm[row][nseg][parts], seg_cmp[row][nseg].
__global__ __launch_bounds__(256) void k_cx_dist(int R, int parts, int ppad, int nseg, const int *__restrict__ seg_word,
                                                 const ulonglong4 *__restrict__ planes, const u64 *__restrict__ pp,
                                                 const u64 *__restrict__ mask, int *__restrict__ mm, int *__restrict__ seg_cmp)
{
    const int lane = threadIdx.x & 63, p0 = blockIdx.y * RP_TP, seg = blockIdx.z;
    const int group = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));   // the same for the wave, and known to be
    if (group * 64 >= R) return;
    const int row = group * 64 + lane, w_lo = seg_word[seg], w_hi = seg_word[seg + 1];
    const bool has = row < R;
    int m[RP_TP], cmp = 0;
#pragma unroll
    for (int a = 0; a < RP_TP; ++a) m[a] = 0;
    for (int w = w_lo; w < w_hi; ++w) {
        // the row's four words are 32 neighbouring bytes, a wave's 2 KB; a thread without a row loads nothing and is valid nowhere
        const ulonglong4 r = has ? planes[(size_t)w * R + row] : make_ulonglong4(0, 0, 0, 0);
        const u64 rv = r.x & mask[w], r0 = r.y, r1 = r.z, r2 = r.w;
        const u64 *q = pp + (size_t)w * 3 * ppad + p0;                 // (the same address in every lane: scalar loads)
        cmp += __popcll(rv);
#pragma unroll
        for (int a = 0; a < RP_TP; ++a) m[a] += __popcll(((r0 ^ q[a]) | (r1 ^ q[ppad + a]) | (r2 ^ q[2 * (size_t)ppad + a])) & rv);
    }
    if (!has) return;
    int *at = mm + ((size_t)row * nseg + seg) * parts + p0;
#pragma unroll
    for (int a = 0; a < RP_TP; ++a)
        if (p0 + a < parts) at[a] = m[a];                              // a slot without a part stores nothing
    if (blockIdx.y == 0) seg_cmp[(size_t)row * nseg + seg] = cmp;
}

// (value, index) as one key whose order is the lexicographic one; values are counts of columns, never negative
#define CX_NONE (~0ull)
__device__ __forceinline__ u64 cx_key(int value, int index) { return ((u64)(unsigned int)value << 32) | (unsigned int)index; }
__device__ __forceinline__ u64 cx_wave_min(u64 k)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(k, d, 64);
        k = o < k ? o : k;
    }
    return k;
}

// grid (rows / 4), 256 threads: a wave per row.  per_row = compared, best, second, the two counts (k_cx_best), then
// cross_split, cross_left, cross_right, cross_mismatches, cross_left_compared, R each.
__global__ __launch_bounds__(256) void k_cx_cross(int R, int parts, int nseg, int min_side, int *__restrict__ mm,
                                                  const int *__restrict__ seg_cmp, int *__restrict__ seg_best, int *__restrict__ per_row)
{
    const int lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (row >= R) return;                                              // (the same for the whole wave)
    int *pre = mm + (size_t)row * nseg * parts;
    const int *cmp = seg_cmp + (size_t)row * nseg;                     // (the same address in every lane)

    // per segment the first smallest count; the counts become prefix sums over the segments
    int total_cmp = 0;
    for (int s = 0; s < nseg; ++s) {
        int *cur = pre + (size_t)s * parts;
        const int *prev = s > 0 ? cur - parts : cur;                   // (read for s > 0 only)
        u64 k = CX_NONE;
        for (int p = lane; p < parts; p += 64) {
            const int v = cur[p];
            const u64 x = cx_key(v, p);
            k = x < k ? x : k;
            if (s > 0) cur[p] = v + prev[p];
        }
        k = cx_wave_min(k);
        if (lane == 0) seg_best[(size_t)row * nseg + s] = cmp[s] > 0 ? (int)(unsigned int)k : -1;
        total_cmp += cmp[s];
    }

    int split = -1, left = -1, right = -1, total = 0, left_cmp = 0;
    if (parts >= 2) {
        const int *last = pre + (size_t)(nseg - 1) * parts;
        int before = 0;                                                // compared columns in the segments < k
        for (int k = 1; k < nseg; ++k) {
            before += cmp[k - 1];
            if (before < min_side || total_cmp - before < min_side) continue;   // not admissible (the same for the whole wave)
            const int *lk = pre + (size_t)(k - 1) * parts;
            // R[k][.]: the first smallest and the first smallest among the others, first within the lane (ascending parts)
            u64 b1 = CX_NONE, b2 = CX_NONE;
            for (int p = lane; p < parts; p += 64) {
                const u64 x = cx_key(last[p] - lk[p], p);
                if (x < b1) { b2 = b1; b1 = x; }
                else if (x < b2) b2 = x;
            }
            const u64 first = cx_wave_min(b1);
            const u64 other = cx_wave_min(b1 == first ? b2 : b1);      // the winner's lane offers its second, every other lane its best
            const int fb = (int)(unsigned int)first, fr = (int)(first >> 32), ob = (int)(unsigned int)other, orr = (int)(other >> 32);
            u64 t = CX_NONE;
            for (int a = lane; a < parts; a += 64) {
                const u64 x = cx_key(lk[a] + (a != fb ? fr : orr), a);
                t = x < t ? x : t;
            }
            t = cx_wave_min(t);
            const int tt = (int)(t >> 32), a = (int)(unsigned int)t;
            if (split < 0 || tt < total) { split = k; left = a; right = a != fb ? fb : ob; total = tt; left_cmp = before; }
        }
    }
    if (lane == 0) {
        int *o = per_row + 5 * (size_t)R + row;
        o[0] = split; o[(size_t)R] = left; o[2 * (size_t)R] = right; o[3 * (size_t)R] = total; o[4 * (size_t)R] = left_cmp;
    }
}

// a thread per row: the one-copy fields from the last prefix row (k_as_best of pgr_assign_device.hip on the sums over all segments)
__global__ __launch_bounds__(256) void k_cx_best(int R, int parts, int nseg, const int *__restrict__ mm, const int *__restrict__ seg_cmp,
                                                 int *__restrict__ per_row)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int compared = 0;
    for (int s = 0; s < nseg; ++s) compared += seg_cmp[(size_t)r * nseg + s];
    const BestSecond x = best_and_second(mm + ((size_t)r * nseg + nseg - 1) * parts, parts, compared);
    per_row[r] = compared; per_row[(size_t)R + r] = x.b; per_row[2 * (size_t)R + r] = x.s;
    per_row[3 * (size_t)R + r] = x.b < 0 ? 0 : x.bm; per_row[4 * (size_t)R + r] = x.s < 0 ? 0 : x.sm;
}

extern "C" void pgr_crossovers_free(pgr_crossovers *o)
{
    if (!o) return;
    free(o->compared); free(o->best); free(o->second); free(o->best_mismatches); free(o->second_mismatches);
    free(o->seg_compared); free(o->seg_best);
    free(o->cross_split); free(o->cross_left); free(o->cross_right); free(o->cross_mismatches); free(o->cross_left_compared);
    free(o->seg_mismatches);
    memset(o, 0, sizeof *o);
}

extern "C" int pgr_last_crossover_timing(double *ms6)
{
    if (!ms6) return PWR_ERR_ARG;
    for (int i = 0; i < 6; ++i) ms6[i] = g_cx_ms[i];
    return PWR_OK;
}

namespace {
// the device buffers of one range of rows
struct Range {
    ulonglong4 *planes = nullptr;
    int *mm = nullptr, *seg_cmp = nullptr, *seg_best = nullptr, *per_row = nullptr;
    DevArena mem;
    bool get(size_t R, size_t nw, size_t nseg, size_t parts)
    {
        planes = mem.get<ulonglong4>(nw * R); mm = mem.get<int>(R * nseg * parts);
        seg_cmp = mem.get<int>(R * nseg); seg_best = mem.get<int>(R * nseg); per_row = mem.get<int>(CX_ROW_INTS * R);
        return planes && mm && seg_cmp && seg_best && per_row;
    }
};
}

static int crossovers(const pgr_msa *h, int parts, int von, int width, const unsigned char *codes, int ncolumns, const int *columns,
                      int nseg, const int *seg_end, int min_side, int want_matrix, pgr_crossovers *o)
{
    const double t0 = now_ms();
    const int rows = h->rows;
    if (parts < 1 || width < 1 || ncolumns < 1 || von < 0 || (long long)von + width > h->width) return PWR_ERR_ARG;   // as pgr_msa_assign
    if (nseg < 1 || min_side < 1) return PWR_ERR_ARG;
    if (parts > PGR_MAX_ROWS || nseg > PGR_CX_MAX_SEGMENTS) return PWR_ERR_RANGE;
    for (int j = 0; j < ncolumns; ++j)
        if (columns[j] < von || columns[j] > von + width - 1 || (j > 0 && columns[j] <= columns[j - 1])) return PWR_ERR_ARG;
    for (int s = 0; s < nseg; ++s)
        if (seg_end[s] <= (s > 0 ? seg_end[s - 1] : 0)) return PWR_ERR_ARG;
    if (seg_end[nseg - 1] != ncolumns) return PWR_ERR_ARG;
    unsigned int above = 0;                                            // (no early exit: the loop is vectorised)
    for (size_t i = 0, n = (size_t)parts * width; i < n; ++i) above |= codes[i] > 4;
    if (above) return PWR_ERR_ARG;

    const size_t T = rows > 0 ? (size_t)rows : 1, S = (size_t)nseg;
    o->rows = rows; o->parts = parts; o->ncolumns = ncolumns; o->nseg = nseg;
    int **per_row[CX_ROW_INTS] = {&o->compared, &o->best, &o->second, &o->best_mismatches, &o->second_mismatches,
                                  &o->cross_split, &o->cross_left, &o->cross_right, &o->cross_mismatches, &o->cross_left_compared};
    for (int **p : per_row)
        if (!(*p = (int *)malloc(sizeof(int) * T))) return PWR_ERR_NOMEM;
    if (!(o->seg_compared = (int *)malloc(sizeof(int) * T * S)) || !(o->seg_best = (int *)malloc(sizeof(int) * T * S))) return PWR_ERR_NOMEM;
    if (want_matrix && !(o->seg_mismatches = (int *)malloc(sizeof(int) * T * S * parts))) return PWR_ERR_NOMEM;

    // the padded column list: every segment starts on a word of 64 entries, a padding entry repeats the segment's last column and
    // mask[word] clears it; seg_word[s] = the first word of segment s
    std::vector<int> seg_word(S + 1, 0);
    for (int s = 0; s < nseg; ++s) seg_word[s + 1] = seg_word[s] + (seg_end[s] - (s > 0 ? seg_end[s - 1] : 0) + 63) / 64;
    const int nw = seg_word[S];
    std::vector<int> padded((size_t)nw * 64);
    std::vector<u64> mask((size_t)nw, 0ull);
    for (int s = 0; s < nseg; ++s) {
        const int lo = s > 0 ? seg_end[s - 1] : 0, n = seg_end[s] - lo;
        for (int i = 0, e = (seg_word[s + 1] - seg_word[s]) * 64; i < e; ++i) {
            padded[(size_t)seg_word[s] * 64 + i] = columns[lo + std::min(i, n - 1)];
            if (i < n) mask[(size_t)seg_word[s] + i / 64] |= 1ull << (i & 63);
        }
    }
    // the parts' three bit planes over the padded list: pp[word][plane][part]
    const int ppad = (parts + RP_TP - 1) / RP_TP * RP_TP;              // whole tiles: the padding stays zero
    std::vector<u64> pp((size_t)nw * 3 * ppad, 0ull);
    for (int p = 0; p < parts; ++p) {
        const unsigned char *c = codes + (size_t)p * width;
        for (int w = 0; w < nw; ++w) {
            u64 b0 = 0, b1 = 0, b2 = 0;
            for (int i = 0; i < 64; ++i) {
                const u64 x = c[padded[(size_t)w * 64 + i] - von];
                b0 |= (x & 1) << i; b1 |= ((x >> 1) & 1) << i; b2 |= (x >> 2) << i;
            }
            u64 *at = &pp[(size_t)w * 3 * ppad + p];
            at[0] = b0; at[ppad] = b1; at[2 * (size_t)ppad] = b2;
        }
    }

    if (hipSetDevice(h->device) != hipSuccess) return PWR_ERR_DEVICE;
    DevArena mem;
    int *d_columns = mem.put(padded.data(), padded.size());
    int *d_seg_word = mem.put(seg_word.data(), seg_word.size());
    u64 *d_mask = mem.put(mask.data(), mask.size());
    u64 *d_pp = mem.put(pp.data(), pp.size());
    if (!d_columns || !d_seg_word || !d_mask || !d_pp) return mem.err;

    // the longest range of rows whose buffers stay within PGR_AS_SCRATCH_BYTES (one row at least) and fit the device
    const long long per = (long long)PGR_AS_SCRATCH_BYTES / (32LL * nw + 4LL * nseg * parts + 8LL * nseg + 4LL * CX_ROW_INTS);
    int R = (int)std::max(1LL, std::min((long long)rows, per));
    std::optional<Range> rg;
    if (const int rc = largest_that_fits(R, [&](int n) { return rg.emplace().get((size_t)n, (size_t)nw, S, (size_t)parts); })) return rc;
    HIPC(hipDeviceSynchronize());
    double t = now_ms(), u;
    g_cx_ms[1] = t - t0; g_cx_ms[2] = g_cx_ms[3] = g_cx_ms[4] = g_cx_ms[5] = 0;

    for (int r_lo = 0; r_lo < rows; r_lo += R) {
        const int n = std::min(R, rows - r_lo);                        // rows of this range; the buffers are laid out for n, not R
        hipLaunchKernelGGL(k_cx_planes, dim3(nw, (n + 255) / 256), dim3(256), 0, 0, (long long)h->width, r_lo, n, nw * 64,
                           (const unsigned char *)h->text, (const int *)d_columns, rg->planes);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_cx_ms[2] += u - t; t = u;
        hipLaunchKernelGGL(k_cx_dist, dim3((n + 255) / 256, ppad / RP_TP, nseg), dim3(256), 0, 0, n, parts, ppad, nseg, (const int *)d_seg_word,
                           (const ulonglong4 *)rg->planes, (const u64 *)d_pp, (const u64 *)d_mask, rg->mm, rg->seg_cmp);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_cx_ms[3] += u - t; t = u;
        if (want_matrix) {                                             // before the counts become prefix sums
            HIPC(hipMemcpy(o->seg_mismatches + (size_t)r_lo * S * parts, rg->mm, sizeof(int) * (size_t)n * S * parts, hipMemcpyDeviceToHost));
            u = now_ms(); g_cx_ms[5] += u - t; t = u;
        }
        hipLaunchKernelGGL(k_cx_cross, dim3((n + 3) / 4), dim3(256), 0, 0, n, parts, nseg, min_side, rg->mm, (const int *)rg->seg_cmp,
                           rg->seg_best, rg->per_row);
        HIPC(hipGetLastError());
        hipLaunchKernelGGL(k_cx_best, dim3((n + 255) / 256), dim3(256), 0, 0, n, parts, nseg, (const int *)rg->mm, (const int *)rg->seg_cmp,
                           rg->per_row);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_cx_ms[4] += u - t; t = u;
        for (int i = 0; i < CX_ROW_INTS; ++i)
            HIPC(hipMemcpy(*per_row[i] + r_lo, rg->per_row + (size_t)i * n, sizeof(int) * n, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(o->seg_compared + (size_t)r_lo * S, rg->seg_cmp, sizeof(int) * (size_t)n * S, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(o->seg_best + (size_t)r_lo * S, rg->seg_best, sizeof(int) * (size_t)n * S, hipMemcpyDeviceToHost));
        u = now_ms(); g_cx_ms[5] += u - t; t = u;
    }
    g_cx_ms[0] = t - t0;
    return PWR_OK;
}

extern "C" int pgr_msa_crossovers(pgr_msa *h, int parts, int von, int width, const unsigned char *codes, int ncolumns, const int *columns,
                                  int nseg, const int *seg_end, int min_side, int want_matrix, pgr_crossovers *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!h || !codes || !columns || !seg_end) return PWR_ERR_ARG;
    const int rc = abi_guard([&] {
        return crossovers(h, parts, von, width, codes, ncolumns, columns, nseg, seg_end, min_side, want_matrix, out);
    });
    if (rc) pgr_crossovers_free(out);
    return rc;
}
