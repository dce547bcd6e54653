// pgr_cons_device.hip -- MI355X (gfx950): per-part symbol counts, consensus and pairwise consensus differences of a
// labelling of the rows of a device-resident MSA, behind include/pgr.h (pgr_msa_consensus).
//
// Reference: PhilippBongartz/RepeatResolver, TransposonAssessment.py ("TA:"): GroupMaker (TA:159-160), Konsensus (TA:82-92),
// SignaturesMaker (TA:156-157) and Diff (TA:94-95); the semantics are restated in the header.
//   k_cs_counts     a work-group per (tile of PGR_CS_TILE window columns, chunk of at most PGR_CS_ROWS rows of one part).  A
//                   thread owns four neighbouring columns: per row one 32-bit word (two aligned loads and a byte shift, since
//                   neither the row stride nor von is a multiple of four), compared against the ten symbols four bytes at a
//                   time; the five counts of its four columns are five words of four 8-bit counters (a chunk has at most 255
//                   rows), unpacked once at the end.  A part of one chunk stores its 20 counts as they are (80 contiguous
//                   bytes per thread); a longer part adds them to counts[part][column][5] with integer atomics (zeros are
//                   not sent).  The rows of a part come from order[], the rows sorted by part on the host.
//   k_cs_consensus  a thread per (part, column of the range): the first code with the largest count, and the depth.
//   k_cs_diff       a wave per pair of parts p < q: the columns of the range in which the two consensus differ, four per
//                   word, once under the selection mask and once without; added to both halves of the matrices.
// The counts of a range of columns are parts * columns * 5 ints: a window whose counts exceed PGR_CS_SCRATCH_INTS (or what the
// device still has) is worked through in ranges of whole tiles; the diff matrices add up over the ranges.
// Every index into the text is 64-bit: rows * width exceeds 2^31 at the size of a real data set.
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

#define CS_THREADS (PGR_CS_TILE / 4)
static_assert(CS_THREADS == 256 && PGR_CS_ROWS <= 255, "four columns per thread, 8-bit counters per chunk");

static double g_cs_ms[5] = {0, 0, 0, 0, 0};

// 0x80 in every byte of x that is zero, 0 in the others (exact: no carry crosses a byte)
__device__ __forceinline__ unsigned int zero_bytes(unsigned int x)
{
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// grid (tiles of the range, chunks); chunk[4 * j] = {part, first entry of order[], entries, 1: the part's only chunk}.  words = the text as aligned 32-bit
// words, nwords of them allocated (pgr_msa_open pads the text to a whole word).  Column c of the range is window column c_lo + c.
__global__ __launch_bounds__(CS_THREADS) void k_cs_counts(long long width, long long nwords, int von, int W, int c_lo, int cw,
                                                          const unsigned int *__restrict__ words, const int *__restrict__ order,
                                                          const int *__restrict__ chunk, int *__restrict__ counts)
{
    const int cr = blockIdx.x * PGR_CS_TILE + 4 * (int)threadIdx.x;    // first of this thread's columns, within the range
    const int nb = min(4, W - (c_lo + cr));                            // how many of the four are inside the window
    if (nb <= 0) return;
    const int4 ch = reinterpret_cast<const int4 *>(chunk)[blockIdx.y];
    const int part = ch.x, begin = ch.y, n = ch.z;
    const unsigned int valid = nb == 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
    const long long tile0 = (long long)von + c_lo + (long long)blockIdx.x * PGR_CS_TILE;   // (the same for the whole work-group)
    unsigned int acc[5] = {0, 0, 0, 0, 0};
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const long long a = (long long)order[begin + i] * width + tile0;   // byte address of the tile's first column in this row
        const int shift = (int)(a & 3);
        const long long idx = (a >> 2) + threadIdx.x;
        // Both loads without a condition, so that the loads of the next rows are issued before these are used.  idx < nwords: the
        // thread's first column is in the window, so in the text.  Where idx + 1 is clamped, the bytes it stands for lie behind
        // the text, so behind the window, and `valid` drops them; with shift == 0 the shift drops all of hi.
        const unsigned int lo = words[idx];
        const unsigned int hi = words[min(idx + 1, nwords - 1)];
        const unsigned int w = (unsigned int)((((unsigned long long)hi << 32) | lo) >> (8 * shift)) & valid;   // (0 is a blank)
        const unsigned int f = w | 0x20202020u;                        // a letter in lower case; no other byte becomes one of a c g t
        acc[0] += zero_bytes(f ^ 0x61616161u) >> 7;                    // a A
        acc[1] += zero_bytes(f ^ 0x63636363u) >> 7;                    // c C
        acc[2] += zero_bytes(f ^ 0x67676767u) >> 7;                    // g G
        acc[3] += zero_bytes(f ^ 0x74747474u) >> 7;                    // t T
        acc[4] += (zero_bytes(w ^ 0x2d2d2d2du) | zero_bytes(w ^ 0x5f5f5f5fu)) >> 7;   // - _
    }
    int *out = counts + ((size_t)part * cw + cr) * 5;                  // (16-byte aligned: cr is a multiple of 4, cw of 1024)
    if (ch.w && nb == 4) {                                             // the part's only chunk: nothing to add to
        int v[20];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 5; ++k) v[j * 5 + k] = (acc[k] >> (8 * j)) & 0xff;
#pragma unroll
        for (int q = 0; q < 5; ++q) reinterpret_cast<int4 *>(out)[q] = make_int4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        return;
    }
    for (int j = 0; j < nb; ++j)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int v = (acc[k] >> (8 * j)) & 0xff;
            if (v) atomicAdd(&out[j * 5 + k], v);                      // (onto the zeros of the memset)
        }
}

// grid (cw / 256, parts): Konsensus (TA:82-92) of every column of the range; the columns behind the window get code 0, so that
// k_cs_diff reads whole words
__global__ __launch_bounds__(256) void k_cs_consensus(int W, int c_lo, int cw, const int *__restrict__ counts,
                                                      unsigned char *__restrict__ cons, int *__restrict__ depth)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (c >= cw) return;
    const size_t at = (size_t)p * cw + c;
    if (c_lo + c >= W) { cons[at] = 0; return; }
    int best = 0, most = counts[at * 5], sum = most;
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const int v = counts[at * 5 + k];
        sum += v;
        if (v > most) { most = v; best = k; }                          // the first maximum: np.argmax (TA:91)
    }
    cons[at] = (unsigned char)best;
    depth[at] = sum;
}

// grid (parts / 4, parts), a wave per pair (p, q), p < q: nw words of four consensus codes; sel[c] = 0x80 for a selected column
__global__ __launch_bounds__(256) void k_cs_diff(int parts, int cw, int nw, const unsigned int *__restrict__ cons,
                                                 const unsigned int *__restrict__ sel, int *__restrict__ diff, int *__restrict__ diff_all)
{
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6), p = blockIdx.y;
    if (q <= p || q >= parts) return;                                  // (the same for the whole wave)
    const unsigned int *A = cons + (size_t)p * (cw / 4), *B = cons + (size_t)q * (cw / 4);
    int all = 0, some = 0;
    for (int i = lane; i < nw; i += 64) {
        const unsigned int x = A[i] ^ B[i];
        const unsigned int nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;   // 0x80 where the codes differ (TA:95)
        all += __popc(nz);
        some += __popc(nz & sel[i]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { all += __shfl_xor(all, d, 64); some += __shfl_xor(some, d, 64); }
    if (lane == 0) {                                                   // (one wave per pair, the ranges one after the other)
        diff_all[(size_t)p * parts + q] += all; diff_all[(size_t)q * parts + p] += all;
        diff[(size_t)p * parts + q] += some; diff[(size_t)q * parts + p] += some;
    }
}

extern "C" void pgr_consensus_free(pgr_consensus *o)
{
    if (!o) return;
    free(o->part_label); free(o->part_rows); free(o->consensus); free(o->depth); free(o->counts); free(o->selected);
    free(o->diff); free(o->diff_all);
    memset(o, 0, sizeof *o);
}

extern "C" int pgr_last_consensus_timing(double *ms5)
{
    if (!ms5) return PWR_ERR_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = g_cs_ms[i];
    return PWR_OK;
}

namespace {
// the device buffers of one range of columns
struct Range {
    int *counts = nullptr, *depth = nullptr;
    unsigned char *cons = nullptr, *sel = nullptr;
    DevArena mem;
    bool get(size_t parts, size_t cw)
    {
        counts = mem.get<int>(parts * cw * 5); depth = mem.get<int>(parts * cw);
        cons = mem.get<unsigned char>(parts * cw); sel = mem.get<unsigned char>(cw);
        return counts && depth && cons && sel;
    }
};
}

static int consensus(const pgr_msa *h, const int *labels, int von, int bis, const double *maxcorrs_full, double cutoff, int want_counts,
                     pgr_consensus *o)
{
    const int rows = h->rows, width = h->width;
    const double t0 = now_ms();
    const int top = pgr_window_and_top(labels, rows, width, &von, &bis);
    if (top < 0) return top;
    const int W = bis + 1 - von;

    // GroupMaker (TA:159-160): the labels that occur, ascending; the rows counting-sorted by part
    std::vector<int> size((size_t)top + 1, 0), part_of((size_t)top + 1, -1);
    for (int r = 0; r < rows; ++r) if (labels[r] >= 0) ++size[labels[r]];
    std::vector<int> label, offset(1, 0);
    for (int x = 0; x <= top; ++x)
        if (size[x] > 0) { part_of[x] = (int)label.size(); label.push_back(x); offset.push_back(offset.back() + size[x]); }
    const int P = (int)label.size();
    std::vector<int> order((size_t)offset[P]), fill(offset.begin(), offset.end() - 1), chunk;
    for (int r = 0; r < rows; ++r) if (labels[r] >= 0) order[fill[part_of[labels[r]]]++] = r;
    for (int p = 0; p < P; ++p)
        for (int b = offset[p]; b < offset[p + 1]; b += PGR_CS_ROWS) {
            chunk.push_back(p); chunk.push_back(b); chunk.push_back(std::min(PGR_CS_ROWS, offset[p + 1] - b));
            chunk.push_back(offset[p + 1] - offset[p] <= PGR_CS_ROWS);
        }
    const int nchunks = (int)(chunk.size() / 4);

    const std::vector<int> selected = pgr_signature_columns(von, bis, maxcorrs_full, cutoff);

    const size_t PW = (size_t)P * W, PP = (size_t)P * P;
    o->rows = rows; o->von = von; o->bis = bis; o->width = W; o->parts = P; o->nselected = (int)selected.size();
    o->part_label = (int *)malloc(sizeof(int) * P); o->part_rows = (int *)malloc(sizeof(int) * P);
    o->consensus = (unsigned char *)malloc(PW); o->depth = (int *)malloc(sizeof(int) * PW);
    o->counts = want_counts ? (int *)malloc(sizeof(int) * PW * 5) : nullptr;
    o->selected = (int *)malloc(sizeof(int) * (selected.size() ? selected.size() : 1));
    o->diff = (int *)malloc(sizeof(int) * PP); o->diff_all = (int *)malloc(sizeof(int) * PP);
    if (!o->part_label || !o->part_rows || !o->consensus || !o->depth || (want_counts && !o->counts) || !o->selected || !o->diff ||
        !o->diff_all)
        return PWR_ERR_NOMEM;
    for (int p = 0; p < P; ++p) { o->part_label[p] = label[p]; o->part_rows[p] = offset[p + 1] - offset[p]; }
    if (!selected.empty()) memcpy(o->selected, selected.data(), sizeof(int) * selected.size());

    if (hipSetDevice(h->device) != hipSuccess) return PWR_ERR_DEVICE;
    DevArena mem;
    int *d_order = mem.put(order.data(), order.size()), *d_chunk = mem.put(chunk.data(), chunk.size());
    int *d_diff = mem.get<int>(PP), *d_all = mem.get<int>(PP);
    if (!d_order || !d_chunk || !d_diff || !d_all) return mem.err;
    HIPC(hipMemset(d_diff, 0, PP * sizeof(int)));
    HIPC(hipMemset(d_all, 0, PP * sizeof(int)));

    // the widest range of whole tiles whose counts stay within PGR_CS_SCRATCH_INTS (one tile at least) and fit the device
    const int tiles = (W + PGR_CS_TILE - 1) / PGR_CS_TILE;
    long long per = (long long)PGR_CS_SCRATCH_INTS / ((long long)P * 5 * PGR_CS_TILE);
    int rt = (int)std::max(1LL, std::min((long long)tiles, per));
    std::optional<Range> rg;
    if (const int rc = largest_that_fits(rt, [&](int n) { return rg.emplace().get((size_t)P, (size_t)n * PGR_CS_TILE); })) return rc;
    const int cw = rt * PGR_CS_TILE;
    HIPC(hipDeviceSynchronize());
    double t = now_ms(), u;
    g_cs_ms[1] = t - t0; g_cs_ms[2] = g_cs_ms[3] = g_cs_ms[4] = 0;

    const long long nwords = ((long long)rows * width + 3) / 4;
    std::vector<unsigned char> sel((size_t)cw);
    size_t s = 0;                                                      // the next selected column
    for (int c_lo = 0; c_lo < W; c_lo += cw) {
        const int wr = std::min(cw, W - c_lo);                         // columns of this range inside the window
        std::fill(sel.begin(), sel.end(), 0);
        for (; s < selected.size() && selected[s] - von < c_lo + wr; ++s) sel[(size_t)(selected[s] - von - c_lo)] = 0x80;
        HIPC(hipMemcpy(rg->sel, sel.data(), (size_t)cw, hipMemcpyHostToDevice));
        HIPC(hipMemset(rg->counts, 0, (size_t)P * cw * 5 * sizeof(int)));
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_cs_ms[1] += u - t; t = u;
        hipLaunchKernelGGL(k_cs_counts, dim3((wr + PGR_CS_TILE - 1) / PGR_CS_TILE, nchunks), dim3(CS_THREADS), 0, 0, (long long)width, nwords,
                           von, W, c_lo, cw, (const unsigned int *)h->text, d_order, d_chunk, rg->counts);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_cs_ms[2] += u - t; t = u;
        hipLaunchKernelGGL(k_cs_consensus, dim3(cw / 256, P), dim3(256), 0, 0, W, c_lo, cw, rg->counts, rg->cons, rg->depth);
        HIPC(hipGetLastError());
        if (P > 1) {
            hipLaunchKernelGGL(k_cs_diff, dim3((P + 3) / 4, P), dim3(256), 0, 0, P, cw, (wr + 3) / 4, (const unsigned int *)rg->cons,
                               (const unsigned int *)rg->sel, d_diff, d_all);
            HIPC(hipGetLastError());
        }
        HIPC(hipDeviceSynchronize());
        u = now_ms(); g_cs_ms[3] += u - t; t = u;
        HIPC(hipMemcpy2D(o->consensus + c_lo, (size_t)W, rg->cons, (size_t)cw, (size_t)wr, (size_t)P, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy2D(o->depth + c_lo, (size_t)W * 4, rg->depth, (size_t)cw * 4, (size_t)wr * 4, (size_t)P, hipMemcpyDeviceToHost));
        if (want_counts)
            HIPC(hipMemcpy2D(o->counts + (size_t)c_lo * 5, (size_t)W * 20, rg->counts, (size_t)cw * 20, (size_t)wr * 20, (size_t)P,
                             hipMemcpyDeviceToHost));
        u = now_ms(); g_cs_ms[4] += u - t; t = u;
    }
    HIPC(hipMemcpy(o->diff, d_diff, PP * sizeof(int), hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(o->diff_all, d_all, PP * sizeof(int), hipMemcpyDeviceToHost));
    u = now_ms(); g_cs_ms[4] += u - t;
    g_cs_ms[0] = u - t0;
    return PWR_OK;
}

extern "C" int pgr_msa_consensus(pgr_msa *h, const int *labels, int von, int bis, const double *maxcorrs_full, double cutoff,
                                 int want_counts, pgr_consensus *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!h || !labels) return PWR_ERR_ARG;
    const int rc = abi_guard([&] { return consensus(h, labels, von, bis, maxcorrs_full, cutoff, want_counts, out); });
    if (rc) pgr_consensus_free(out);
    return rc;
}
