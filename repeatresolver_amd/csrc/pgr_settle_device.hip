// pgr_settle_device.hip -- MI355X (gfx950): a labelling of the rows of a device-resident MSA settled on the device, behind
// include/pgr.h (pgr_msa_settle): the consensus of every part (pgr_msa_consensus), every row against them (pgr_msa_assign) and
// the label rule of resolution.Assignment.labels, iterated until no row moves.
//
// The reference (PhilippBongartz/RepeatResolver) has no counterpart: the result is defined by the composition of the two
// existing entries, which the header writes out, and everything is an integer.  The rows' bit planes over the candidate columns
// do not change between iterations, only the labels do: the planes are made once (k_st_planes) and stay resident; an iteration
// reads no text, does no host arithmetic and sends one record of four ints to the host.
//   k_st_planes   once per call: the plane body of row_planes.h (k_as_planes of pgr_assign_device.hip) over all rows:
//                 planes[word][row] = {valid, bit0, bit1, bit2}.  The four words of a (word, row) are 32 neighbouring bytes, and
//                 k_st_cons gathers rows: were they apart, each of the four would cost it a 64-byte line of its own.
//   k_st_hist     per iteration: the rows of every label (integer atomics onto zeros).
//   k_st_scan     one work-group: the labels that occur, ascending, are the parts of this iteration: part_of[label],
//                 part_label[part], the offsets of the parts in order[]; it zeroes the histogram again and starts the record.
//   k_st_scatter  order[]: the rows sorted by part (the place within a part comes from an atomic cursor: counts do not
//                 depend on the order).
//   k_st_cons     a work-group per (word, living part): lane = column, the part's rows through order[]; a row's four plane
//                 words have the same address in every lane, so they are one scalar load and the five symbol masks are made
//                 on the scalar unit; five counters per lane.  The four waves share the part's rows and add up in LDS.  The code
//                 is the first maximum, the depth the sum; ballots of the code's bits are the part's three plane words, a
//                 ballot of depth >= min_depth its column-ok word.
//   k_st_mask     a wave per word: the AND of the living parts' ok words and of the candidate tail; its population count is
//                 added to the record's ncolumns.
//   k_st_dist     the distance body of row_planes.h (k_as_dist) with valid & mask[word], the number of parts from the record.
//   k_st_label    a thread per row: best and second over the living parts (row_planes.h, as k_as_best), the label rule, hold,
//                 the new label; the changed rows by a block count and one integer atomic add.
// A part that has died takes no work: the grids are sized for the parts of the initial labelling (parts are never born)
// and a work-group behind the living parts returns at once.  The per-row results, part_label and mask are kept for two
// iterations (index: iteration & 1), because an iteration that finds no column must leave the one before intact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PWR_STAGE "pgr"
#include "dev_util.h"
#include "pgr.h"
#include "pgr_internal.h"
#include "row_planes.h"

#define ST_CW 4                  // waves of a work-group of k_st_cons: they share the part's rows
#define ST_SCAN 1024             // threads of k_st_scan

// the record of an iteration, the only thing the host reads inside the loop
enum { REC_CHANGED = 0, REC_PARTS = 1, REC_NCOLUMNS = 2, REC_ANY = 3, REC_INTS = 4 };

static double g_st_ms[5] = {0, 0, 0, 0, 0};

// grid (words, groups of 4 x 64 rows), 256 threads: all R rows of the text; planes[word][row]
__global__ __launch_bounds__(256) void k_st_planes(long long width, int R, int ncolumns, const unsigned char *__restrict__ text,
                                                   const int *__restrict__ columns, ulonglong4 *__restrict__ planes)
{
    row_planes_group(width, 0, R, ncolumns, text, columns, planes);
}

// a thread per row: size[label] += 1 (onto the zeros k_st_scan leaves)
__global__ __launch_bounds__(256) void k_st_hist(int R, const int *__restrict__ lab, int *__restrict__ size)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R && lab[r] >= 0) atomicAdd(&size[lab[r]], 1);
}

// one work-group of ST_SCAN threads over the L label values, a run of neighbouring labels per thread: the labels that occur
// become the parts 0, 1, ... in ascending order.  offset[parts + 1], cursor[parts] = offset; size[] is zero again afterwards.
__global__ __launch_bounds__(ST_SCAN) void k_st_scan(int L, int *__restrict__ size, int *__restrict__ part_of, int *__restrict__ part_label,
                                                     int *__restrict__ offset, int *__restrict__ cursor, int *__restrict__ rec)
{
    __shared__ int alive[ST_SCAN], total[ST_SCAN];
    const int t = threadIdx.x, per = (L + ST_SCAN - 1) / ST_SCAN, lo = min(L, t * per), hi = min(L, lo + per);
    int a = 0, n = 0;
    for (int l = lo; l < hi; ++l) { a += size[l] > 0; n += size[l]; }
    alive[t] = a; total[t] = n;
    __syncthreads();
    for (int d = 1; d < ST_SCAN; d <<= 1) {                            // inclusive scans of both
        const int xa = t >= d ? alive[t - d] : 0, xn = t >= d ? total[t - d] : 0;
        __syncthreads();
        alive[t] += xa; total[t] += xn;
        __syncthreads();
    }
    int p = alive[t] - a, at = total[t] - n;                           // exclusive: the first part and the first entry of this run
    for (int l = lo; l < hi; ++l) {
        const int s = size[l];
        part_of[l] = s > 0 ? p : -1;
        if (s > 0) { part_label[p] = l; offset[p] = at; cursor[p] = at; ++p; at += s; }
        size[l] = 0;
    }
    if (t == ST_SCAN - 1) {
        offset[alive[t]] = total[t];
        rec[REC_CHANGED] = 0; rec[REC_PARTS] = alive[t]; rec[REC_NCOLUMNS] = 0; rec[REC_ANY] = 0;
    }
}

// a thread per row: its place in order[]
__global__ __launch_bounds__(256) void k_st_scatter(int R, const int *__restrict__ lab, const int *__restrict__ part_of,
                                                    int *__restrict__ cursor, int *__restrict__ order)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R && lab[r] >= 0) order[atomicAdd(&cursor[part_of[lab[r]]], 1)] = r;
}

// One row's four plane words (the same in every lane) onto the five counters of every lane's column.  The symbols' masks are made
// on the scalar unit; a mask that is the same in every lane is a lane mask as it stands (the inverse of a ballot), so a counter
// costs one select and one add, and no 64-bit shift by the lane.
__device__ __forceinline__ void count_symbols(int (&c)[5], u64 v, u64 x0, u64 x1, u64 x2)
{
    const u64 base = v & ~x2;
    c[0] += __builtin_amdgcn_inverse_ballot_w64(base & ~x1 & ~x0) ? 1 : 0;
    c[1] += __builtin_amdgcn_inverse_ballot_w64(base & ~x1 & x0) ? 1 : 0;
    c[2] += __builtin_amdgcn_inverse_ballot_w64(base & x1 & ~x0) ? 1 : 0;
    c[3] += __builtin_amdgcn_inverse_ballot_w64(base & x1 & x0) ? 1 : 0;
    c[4] += __builtin_amdgcn_inverse_ballot_w64(v & x2) ? 1 : 0;
}

// grid (words, parts of the initial labelling), 64 * ST_CW threads.  pp[word][plane 0..2][ppad] as k_st_dist reads it,
// ok[word][ppad].
__global__ __launch_bounds__(64 * ST_CW) void k_st_cons(int R, int ppad, int min_depth, const int *__restrict__ rec,
                                                        const ulonglong4 *__restrict__ planes, const int *__restrict__ order,
                                                        const int *__restrict__ offset, u64 *__restrict__ pp, u64 *__restrict__ ok)
{
    __shared__ int part[ST_CW - 1][5][64];
    const int p = blockIdx.y, w = blockIdx.x, lane = threadIdx.x & 63;
    if (p >= rec[REC_PARTS]) return;                                   // a part that has died (the same for the whole work-group)
    const int s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = offset[p], n = offset[p + 1] - b, share = (n + ST_CW - 1) / ST_CW;      // wave s: a run of `share` entries of the part
    const int hi = b + min(n, (s + 1) * share);
    const ulonglong4 *pl = planes + (size_t)w * R;
    int c[5] = {0, 0, 0, 0, 0};
    int i = b + min(n, s * share);
    for (; i + 4 <= hi; i += 4) {                                      // four rows at a time: their loads are in flight together
        ulonglong4 q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = pl[order[i + k]];           // (the same address in every lane: scalar loads, 32 bytes of one line)
#pragma unroll
        for (int k = 0; k < 4; ++k) count_symbols(c, q[k].x, q[k].y, q[k].z, q[k].w);
    }
    for (; i < hi; ++i) {
        const ulonglong4 q = pl[order[i]];
        count_symbols(c, q.x, q.y, q.z, q.w);
    }
    if (s > 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) part[s - 1][k][lane] = c[k];
    __syncthreads();
    if (s > 0) return;
#pragma unroll
    for (int o = 0; o < ST_CW - 1; ++o)
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] += part[o][k][lane];
    int code = 0, most = c[0], depth = c[0];
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        depth += c[k];
        if (c[k] > most) { most = c[k]; code = k; }                    // the first maximum: a before c, any base before '-'
    }
    const u64 b0 = __ballot(code & 1), b1 = __ballot(code & 2), b2 = __ballot(code & 4), good = __ballot(depth >= min_depth);
    if (lane == 0) {
        u64 *q = pp + (size_t)w * 3 * ppad + p;
        q[0] = b0; q[ppad] = b1; q[2 * (size_t)ppad] = b2;
        ok[(size_t)w * ppad + p] = good;
    }
}

// grid (words / 4), 256 threads, a wave per word
__global__ __launch_bounds__(256) void k_st_mask(int nw, int ncandidates, int ppad, const u64 *__restrict__ ok, u64 *__restrict__ mask,
                                                 int *__restrict__ rec)
{
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (w >= nw) return;                                               // (the same for the whole wave)
    const int parts = rec[REC_PARTS];
    u64 m = ~0ull;
    for (int p = lane; p < parts; p += 64) m &= ok[(size_t)w * ppad + p];
    unsigned int lo = (unsigned int)m, hi = (unsigned int)(m >> 32);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { lo &= __shfl_xor(lo, d, 64); hi &= __shfl_xor(hi, d, 64); }
    m = ((u64)hi << 32) | lo;
    if (w == nw - 1 && (ncandidates & 63)) m &= (1ull << (ncandidates & 63)) - 1ull;   // the candidates end inside the last word
    if (lane == 0) {
        mask[w] = m;
        if (m) atomicAdd(&rec[REC_NCOLUMNS], __popcll(m));
    }
}

// grid (R / RP_ROWS, tiles of the initial parts), 64 * RP_NW threads: the row's valid word under mask[word]; mat[row][ppad]
__global__ __launch_bounds__(64 * RP_NW) void k_st_dist(int R, int ppad, int nw, const int *__restrict__ rec,
                                                        const ulonglong4 *__restrict__ planes, const u64 *__restrict__ pp,
                                                        const u64 *__restrict__ mask, int *__restrict__ mat,
                                                        int *__restrict__ compared)
{
    const int parts = rec[REC_PARTS];
    if ((int)blockIdx.y * RP_TP >= parts || rec[REC_NCOLUMNS] == 0) return;   // a tile of dead parts, or no column (the same for the whole work-group)
    __builtin_assume(mask != nullptr);                                 // (so that the body's test of it goes, as with k_as_dist's literal)
    row_part_distances(R, parts, ppad, ppad, nw, planes, pp, mask, mat, compared);
}

// a thread per row; per_row = compared, best, second and the two counts of this iteration, R each.  init = the initial labels
// where they hold, else null.
__global__ __launch_bounds__(256) void k_st_label(int R, int ppad, int min_compared, int min_margin, const int *__restrict__ mat,
                                                  const int *__restrict__ part_label, const int *__restrict__ init, const int *__restrict__ cur,
                                                  int *__restrict__ next, int *__restrict__ per_row, int *__restrict__ rec)
{
    if (rec[REC_NCOLUMNS] == 0) return;                                // no column: the labelling stays (the same for the whole grid)
    const int r = blockIdx.x * blockDim.x + threadIdx.x, parts = rec[REC_PARTS];
    int moved = 0, any = 0;
    if (r < R) {
        const int cmp = per_row[r];
        const BestSecond x = best_and_second(mat + (size_t)r * ppad, parts, cmp);
        const int b = x.b, s = x.s, bm = b < 0 ? 0 : x.bm, sm = s < 0 ? 0 : x.sm;
        per_row[(size_t)R + r] = b; per_row[2 * (size_t)R + r] = s; per_row[3 * (size_t)R + r] = bm; per_row[4 * (size_t)R + r] = sm;
        int l = b >= 0 && cmp >= min_compared && (s == -1 || sm - bm >= min_margin) ? part_label[b] : -1;
        if (init && init[r] >= 0) l = init[r];
        next[r] = l;
        moved = l != cur[r]; any = l >= 0;
    }
    const int n = __syncthreads_count(moved), some = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        if (n) atomicAdd(&rec[REC_CHANGED], n);
        if (some) atomicOr(&rec[REC_ANY], 1);
    }
}

extern "C" void pgr_settlement_free(pgr_settlement *o)
{
    if (!o) return;
    free(o->part_label); free(o->labels); free(o->changed); free(o->parts_at); free(o->ncolumns_at); free(o->columns);
    free(o->compared); free(o->best); free(o->second); free(o->best_mismatches); free(o->second_mismatches);
    memset(o, 0, sizeof *o);
}

extern "C" int pgr_last_settle_timing(double *ms5)
{
    if (!ms5) return PWR_ERR_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = g_st_ms[i];
    return PWR_OK;
}

// a malloc'ed copy of from[n], n >= 1; null when the host has no room
template <class T> static T *host_copy(const T *from, size_t n)
{
    T *p = (T *)malloc(sizeof(T) * n);
    if (p) memcpy(p, from, sizeof(T) * n);
    return p;
}

static int settle(const pgr_msa *h, const int *labels, int von, int bis, const double *maxcorrs_full, double cutoff, int min_depth,
                  int all_columns, int min_compared, int min_margin, int hold, int max_iter, pgr_settlement *o)
{
    const double t0 = now_ms();
    const int rows = h->rows, width = h->width;
    if (max_iter < 1 || min_depth < 1 || min_compared < 0 || min_margin < 0) return PWR_ERR_ARG;
    const int top = pgr_window_and_top(labels, rows, width, &von, &bis);   // as pgr_msa_consensus
    if (top < 0) return top;
    const int L = top + 1;                                             // no label above `top` ever appears: a row takes a part's label or keeps its own
    std::vector<char> seen((size_t)L, 0);
    int P0 = 0;                                                        // the parts of the initial labelling: parts die, none is born
    for (int r = 0; r < rows; ++r)
        if (labels[r] >= 0 && !seen[labels[r]]) { seen[labels[r]] = 1; ++P0; }

    // the candidate columns, fixed for the call: SignaturesMaker's, or the whole window
    const std::vector<int> cand = pgr_signature_columns(von, bis, all_columns ? nullptr : maxcorrs_full, cutoff);
    const int nc = (int)cand.size();

    o->rows = rows;
    if (!(o->labels = host_copy(labels, (size_t)rows))) return PWR_ERR_NOMEM;
    if (nc == 0) {                                                     // no candidate, so no column in iteration 0
        o->stop = PGR_ST_NO_COLUMN;
        g_st_ms[0] = g_st_ms[1] = now_ms() - t0; g_st_ms[2] = g_st_ms[3] = g_st_ms[4] = 0;
        return PWR_OK;
    }

    if (hipSetDevice(h->device) != hipSuccess) return PWR_ERR_DEVICE;
    const size_t R = (size_t)rows;
    const int nw = (nc + 63) / 64, ppad = (P0 + RP_TP - 1) / RP_TP * RP_TP;
    DevArena mem;
    int *d_cand = mem.put(cand.data(), cand.size());
    int *d_lab[2] = {mem.put(labels, R), mem.get<int>(R)};
    int *d_init = hold ? mem.put(labels, R) : nullptr;
    ulonglong4 *d_planes = mem.get<ulonglong4>((size_t)nw * R);
    u64 *d_pp = mem.get<u64>((size_t)nw * 3 * ppad), *d_ok = mem.get<u64>((size_t)nw * ppad), *d_mask = mem.get<u64>(2 * (size_t)nw);
    int *d_mat = mem.get<int>(R * ppad), *d_per_row = mem.get<int>(2 * 5 * R), *d_order = mem.get<int>(R);
    int *d_size = mem.get<int>((size_t)L), *d_part_of = mem.get<int>((size_t)L), *d_part_label = mem.get<int>(2 * (size_t)P0);
    int *d_offset = mem.get<int>((size_t)P0 + 1), *d_cursor = mem.get<int>((size_t)P0), *d_rec = mem.get<int>(REC_INTS);
    if (!d_cand || !d_lab[0] || !d_lab[1] || (hold && !d_init) || !d_planes || !d_pp || !d_ok || !d_mask || !d_mat || !d_per_row ||
        !d_order || !d_size || !d_part_of || !d_part_label || !d_offset || !d_cursor || !d_rec) {
        (void)hipGetLastError();
        return mem.err;
    }
    HIPC(hipMemset(d_size, 0, sizeof(int) * (size_t)L));
    HIPC(hipMemset(d_pp, 0, sizeof(u64) * (size_t)nw * 3 * ppad));      // a slot of a tile behind the living parts is read, never used
    HIPC(hipDeviceSynchronize());
    double t = now_ms(), u;
    g_st_ms[1] = t - t0;

    hipLaunchKernelGGL(k_st_planes, dim3(nw, (rows + 255) / 256), dim3(256), 0, 0, (long long)width, rows, nc, (const unsigned char *)h->text,
                       (const int *)d_cand, d_planes);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    u = now_ms(); g_st_ms[2] = u - t; t = u;

    std::vector<int> changed, parts_at, ncolumns_at;
    int stop = PGR_ST_MAX_ITER, last = -1, cur = 0;                    // last: the iteration whose assignment made the labels returned
    const int rb = (rows + 255) / 256;
    for (int it = 0; it < max_iter; ++it) {
        const int k = it & 1;
        int *per_row = d_per_row + (size_t)k * 5 * R, *part_label = d_part_label + (size_t)k * P0;
        u64 *mask = d_mask + (size_t)k * nw;
        hipLaunchKernelGGL(k_st_hist, dim3(rb), dim3(256), 0, 0, rows, (const int *)d_lab[cur], d_size);
        hipLaunchKernelGGL(k_st_scan, dim3(1), dim3(ST_SCAN), 0, 0, L, d_size, d_part_of, part_label, d_offset, d_cursor, d_rec);
        hipLaunchKernelGGL(k_st_scatter, dim3(rb), dim3(256), 0, 0, rows, (const int *)d_lab[cur], (const int *)d_part_of, d_cursor, d_order);
        hipLaunchKernelGGL(k_st_cons, dim3(nw, P0), dim3(64 * ST_CW), 0, 0, rows, ppad, min_depth, (const int *)d_rec, (const ulonglong4 *)d_planes,
                           (const int *)d_order, (const int *)d_offset, d_pp, d_ok);
        hipLaunchKernelGGL(k_st_mask, dim3((nw + 3) / 4), dim3(256), 0, 0, nw, nc, ppad, (const u64 *)d_ok, mask, d_rec);
        hipLaunchKernelGGL(k_st_dist, dim3((rows + RP_ROWS - 1) / RP_ROWS, ppad / RP_TP), dim3(64 * RP_NW), 0, 0, rows, ppad, nw,
                           (const int *)d_rec, (const ulonglong4 *)d_planes, (const u64 *)d_pp, (const u64 *)mask, d_mat, per_row);
        hipLaunchKernelGGL(k_st_label, dim3(rb), dim3(256), 0, 0, rows, ppad, min_compared, min_margin, (const int *)d_mat,
                           (const int *)part_label, (const int *)d_init, (const int *)d_lab[cur], d_lab[cur ^ 1], per_row, d_rec);
        HIPC(hipGetLastError());
        int rec[REC_INTS];
        HIPC(hipMemcpy(rec, d_rec, sizeof rec, hipMemcpyDeviceToHost));   // (waits for the iteration)
        if (rec[REC_NCOLUMNS] == 0) { stop = PGR_ST_NO_COLUMN; break; }
        changed.push_back(rec[REC_CHANGED]); parts_at.push_back(rec[REC_PARTS]); ncolumns_at.push_back(rec[REC_NCOLUMNS]);
        last = it;
        if (rec[REC_CHANGED] == 0) { stop = PGR_ST_CONVERGED; break; }
        if (!rec[REC_ANY]) { stop = PGR_ST_EMPTY; break; }             // the labelling before stays
        cur ^= 1;
    }
    u = now_ms(); g_st_ms[3] = u - t; t = u;

    o->stop = stop; o->iterations = (int)changed.size();
    if (!changed.empty()) {                                            // (no iteration: the three histories stay NULL)
        o->changed = host_copy(changed.data(), changed.size()); o->parts_at = host_copy(parts_at.data(), parts_at.size());
        o->ncolumns_at = host_copy(ncolumns_at.data(), ncolumns_at.size());
        if (!o->changed || !o->parts_at || !o->ncolumns_at) return PWR_ERR_NOMEM;
    }
    HIPC(hipMemcpy(o->labels, d_lab[cur], sizeof(int) * R, hipMemcpyDeviceToHost));
    if (last >= 0) {
        const int k = last & 1;
        o->parts = parts_at[(size_t)last]; o->ncolumns = ncolumns_at[(size_t)last];
        int **per_row[5] = {&o->compared, &o->best, &o->second, &o->best_mismatches, &o->second_mismatches};
        for (int i = 0; i < 5; ++i) {
            if (!(*per_row[i] = (int *)malloc(sizeof(int) * R))) return PWR_ERR_NOMEM;
            HIPC(hipMemcpy(*per_row[i], d_per_row + ((size_t)k * 5 + i) * R, sizeof(int) * R, hipMemcpyDeviceToHost));
        }
        if (!(o->part_label = (int *)malloc(sizeof(int) * (size_t)o->parts)) || !(o->columns = (int *)malloc(sizeof(int) * (size_t)o->ncolumns)))
            return PWR_ERR_NOMEM;
        HIPC(hipMemcpy(o->part_label, d_part_label + (size_t)k * P0, sizeof(int) * (size_t)o->parts, hipMemcpyDeviceToHost));
        std::vector<u64> mask((size_t)nw);
        HIPC(hipMemcpy(mask.data(), d_mask + (size_t)k * nw, sizeof(u64) * (size_t)nw, hipMemcpyDeviceToHost));
        int n = 0;
        for (int j = 0; j < nc; ++j)
            if ((mask[(size_t)j >> 6] >> (j & 63)) & 1) {
                if (n == o->ncolumns) return PWR_ERR_INTERNAL;
                o->columns[n++] = cand[(size_t)j];
            }
        if (n != o->ncolumns) return PWR_ERR_INTERNAL;
    }
    u = now_ms(); g_st_ms[4] = u - t;
    g_st_ms[0] = u - t0;
    return PWR_OK;
}

extern "C" int pgr_msa_settle(pgr_msa *h, const int *labels, int von, int bis, const double *maxcorrs_full, double cutoff, int min_depth,
                              int all_columns, int min_compared, int min_margin, int hold, int max_iter, pgr_settlement *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!h || !labels) return PWR_ERR_ARG;
    const int rc = abi_guard([&] {
        return settle(h, labels, von, bis, maxcorrs_full, cutoff, min_depth, all_columns, min_compared, min_margin, hold, max_iter, out);
    });
    if (rc) pgr_settlement_free(out);
    return rc;
}
