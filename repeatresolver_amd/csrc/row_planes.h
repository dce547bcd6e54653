// row_planes.h -- the device code k_as_* (pgr_assign_device.hip) and k_st_* (pgr_settle_device.hip) share: the rows of an MSA as
// bit planes over a list of columns, the rows' distances to the parts' planes, and the best and the second part of a row.
// planes[word][row] = {valid, bit0, bit1, bit2}: the four words of 64 columns of a row are 32 neighbouring bytes, which a lane
// of the planes and of the distance body moves in one piece (a wave: 2 KB, contiguous) and which k_st_cons, gathering the rows of
// a part, finds in one 64-byte line.  pp[word][plane 0..2][ppad]: the parts' planes, ppad = the parts rounded up to whole tiles,
// the padding zero, so that no load of a tile needs a condition.
#ifndef PGR_ROW_PLANES_H
#define PGR_ROW_PLANES_H

#include <hip/hip_runtime.h>

#include <climits>

#include "pgr.h"

#define RP_TP PGR_AS_TILE        // parts per tile of the distance body
#define RP_NW 16                 // waves of a work-group of the distance body: they share the words
#define RP_ROWS 64               // rows per work-group of the distance body: one per lane
static_assert(RP_TP == 8, "3 x 8 plane words of a tile are 48 scalar registers; eight counters per thread");

typedef unsigned long long u64;

// grid (words, groups of 4 x 64 rows), 256 threads.  The rows are [r_lo, r_lo + R) of the text, planes[word][row of the R].  A
// wave owns 64 entries of columns[] (one word) and a group of 64 rows, which it reads one after the other; lane i keeps the
// four words of the group's i-th row.
__device__ __forceinline__ void row_planes_group(long long width, int r_lo, int R, int ncolumns, const unsigned char *__restrict__ text,
                                                 const int *__restrict__ columns, ulonglong4 *__restrict__ planes)
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
    if (lane < n) planes[(size_t)w * R + row0 + lane] = make_ulonglong4(keep[0], keep[1], keep[2], keep[3]);   // 2 KB per wave, contiguous
}

// grid (R / RP_ROWS, tiles of parts), 64 * RP_NW threads: lane = the row, wave s = the words w = s mod RP_NW.  The address of a
// part's plane word does not depend on the lane, so the tile's 3 x RP_TP words of a word index come by scalar loads and are
// operands of the vector instructions as they are: no LDS traffic, no barrier inside the loop.  Per (row, part, word)
// d = ((r0 ^ p0) | (r1 ^ p1) | (r2 ^ p2)) & valid, m += popcount(d), where valid is the row's word under mask[word] (mask
// null: every column counts; a literal at the call, so that no test of it is left).  The counters stay in registers; at the
// end every wave puts its counters into LDS and wave j adds up counter j of all waves and stores mat[row][part] (rows of
// `stride` ints), or, for the last counter in the first tile of parts, compared[row] = the popcount of valid.  A slot without a
// part stores nothing.
__device__ __forceinline__ void row_part_distances(int R, int parts, int ppad, int stride, int nw, const ulonglong4 *__restrict__ planes,
                                                   const u64 *__restrict__ pp, const u64 *__restrict__ mask, int *__restrict__ mat,
                                                   int *__restrict__ compared)
{
    __shared__ int red[RP_NW][RP_TP + 1][64];                          // every wave's counters, the last one compared
    const int lane = threadIdx.x & 63, p0 = blockIdx.y * RP_TP, row = blockIdx.x * RP_ROWS + lane;
    const int slice = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // the same for the wave, and known to be: what follows from it is scalar
    const bool has = row < R;
    int m[RP_TP], cmp = 0;
#pragma unroll
    for (int a = 0; a < RP_TP; ++a) m[a] = 0;
    for (int w = slice; w < nw; w += RP_NW) {
        // the row's four words are 32 neighbouring bytes, a wave's 2 KB; a thread without a row loads nothing and is valid nowhere
        const ulonglong4 r = has ? planes[(size_t)w * R + row] : make_ulonglong4(0, 0, 0, 0);
        const u64 rv = mask ? r.x & mask[w] : r.x, r0 = r.y, r1 = r.z, r2 = r.w;
        const u64 *q = pp + (size_t)w * 3 * ppad + p0;                 // (the same address in every lane: scalar loads)
        cmp += __popcll(rv);
#pragma unroll
        for (int a = 0; a < RP_TP; ++a) m[a] += __popcll(((r0 ^ q[a]) | (r1 ^ q[ppad + a]) | (r2 ^ q[2 * (size_t)ppad + a])) & rv);
    }
#pragma unroll
    for (int a = 0; a < RP_TP; ++a) red[slice][a][lane] = m[a];
    red[slice][RP_TP][lane] = cmp;
    __syncthreads();
    for (int j = slice; j <= RP_TP; j += RP_NW) {                      // counter j of all waves, by wave j
        int sum = 0;
#pragma unroll
        for (int o = 0; o < RP_NW; ++o) sum += red[o][j][lane];
        if (!has) continue;
        if (j == RP_TP) { if (blockIdx.y == 0) compared[row] = sum; }
        else if (p0 + j < parts) mat[(size_t)row * stride + p0 + j] = sum;
    }
}

// The first smallest of row[0 .. parts) (b, its value bm) and the first smallest among the others (s, sm); -1 and INT_MAX
// where there is none: for a single part the second, for a row with nothing compared both.
struct BestSecond { int b, s, bm, sm; };
__device__ __forceinline__ BestSecond best_and_second(const int *__restrict__ row, int parts, int compared)
{
    int b = -1, s = -1, bm = INT_MAX, sm = INT_MAX;
    if (compared > 0)
        for (int p = 0; p < parts; ++p) {
            const int v = row[p];
            // the best that is displaced becomes the second: it is smaller than the second, or equal and of lower index
            if (v < bm) { s = b; sm = bm; b = p; bm = v; }
            else if (v < sm) { s = p; sm = v; }
        }
    return {b, s, bm, sm};
}

#endif /* PGR_ROW_PLANES_H */
