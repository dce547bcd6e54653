// pmc_device.hip -- MI355X (gfx950) implementation of MaxCorrelation's pair loop behind include/pmc.h.
//
// Reference: PhilippBongartz/RepeatResolver, MaxCorrelation.c ("MC:"), HilfsMaxCorrsRechner (MC:745-837): for every
// relevant variation i = (column ii, symbol k) and every relevant variation j in the columns jj >= ii + 20, as long as the
// two columns share at least `mincov` rows (the loop ends at the FIRST column that does not, MC:801-804), four sizes of
// intersections of row bit sets (MC:421-426) go into one upper tail of a hypergeometric distribution (MC:413-419, GSL);
// MaxCorrs[i] and MaxCorrs[j] keep the maximum (MC:816-817).
//   k_mc_bits   the bit sets, word-major: G[w][column * 5 + symbol], LC[w][column]  (MC:340-382), group sizes, coverage;
//               rows take their bit positions in the order of their first covered column, so that the rows of a column
//               sit in a narrow range of words (k_mc_colrange) and the products skip the words where a side is all zero
//   k_mc_end    per column the end of its jj loop
//   k_mc_pairs  a tiled bit-set product: a tile of PMC_TI relevant variations i stays in LDS (their group and their
//               column's coverage, a chunk of words at a time), every thread owns one relevant variation j and streams
//               its two bit sets once; the four counts per (i, j) live in registers, the epilogue evaluates the tail
//               in double precision and folds the maxima.
// The tail follows GSL's scheme (sum of pdf terms by ratio recurrences away from k; pdf = exp of three lnchoose): equal to
// the reference's up to rounding of lgamma / exp / log10, not bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define PWR_STAGE "pmc"
#include "base_code.h"
#include "dev_util.h"
#include "four_count_tile.h"
#include "hyper_tail.h"
#include "pmc.h"

#define PMC_TI 16                   // variations i per tile
#define PMC_NT 256                  // threads per block = variations j per tile
#define PMC_WC 32                   // words per LDS chunk
#define PMC_EI 8                    // columns per block of k_mc_end

static double g_ms[5] = {0, 0, 0, 0, 0};

// first covered column of every row (W if it has none): block per row
__global__ __launch_bounds__(256) void k_mc_rowstart(int W, const unsigned char *__restrict__ text, int *__restrict__ start)
{
    __shared__ int s_min;
    if (threadIdx.x == 0) s_min = W;
    __syncthreads();
    const unsigned char *row = text + (size_t)blockIdx.x * W;
    for (int c0 = 0; c0 < W; c0 += 256) {                            // the start is usually near the row's left end
        const int c = c0 + threadIdx.x;
        if (c < W && base_code(row[c]) < 5) atomicMin(&s_min, c);
        __syncthreads();
        if (s_min < W) break;
        __syncthreads();
    }
    if (threadIdx.x == 0) start[blockIdx.x] = s_min;
}

// thread = (column c, word w): 64 bit positions of one column.  The rows take their bit positions in the order of their first
// covered column (inv[position] = row): no count depends on the order, but the rows that cover a column then sit in a narrow
// range of words, and the products below only visit the words where both sides can be non-zero.
__global__ __launch_bounds__(256) void k_mc_bits(int T, int W, int sc, const unsigned char *__restrict__ text, const int *__restrict__ inv,
                                                 unsigned long long *__restrict__ G, unsigned long long *__restrict__ LC,
                                                 int *__restrict__ gsize, int *__restrict__ cover)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    if (c >= W) return;
    unsigned long long g[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < 64; ++r) {
        const int pos = w * 64 + r;
        if (pos >= T) break;
        const int k = base_code(text[(size_t)inv[pos] * W + c]);
        if (k < 5) g[k] |= 1ull << r;
    }
    unsigned long long lc = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        G[(size_t)w * W * 5 + (size_t)c * 5 + k] = g[k];
        lc |= g[k];
        if (g[k]) atomicAdd(&gsize[c * 5 + k], __popcll(g[k]));
    }
    LC[(size_t)w * W + c] = lc;
    if (lc) atomicAdd(&cover[c], __popcll(lc));
}

// the words of a column's coverage set that are not zero: [wlo, whi)
__global__ __launch_bounds__(256) void k_mc_colrange(int W, int sc, const unsigned long long *__restrict__ LC, int2 *__restrict__ wr)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W) return;
    int lo = sc, hi = 0;
    for (int w = 0; w < sc; ++w)
        if (LC[(size_t)w * W + c]) { lo = min(lo, w); hi = w + 1; }
    wr[c] = make_int2(min(lo, hi), hi);
}

// MC:798-804: jend[ii] = the first jj >= ii + 20 whose column shares fewer than mincov rows with column ii (or W)
__global__ __launch_bounds__(256) void k_mc_end(int W, int sc, int mincov, const unsigned long long *__restrict__ LC, const int2 *__restrict__ wr,
                                                int *__restrict__ jend)
{
    extern __shared__ unsigned long long sL[];                         // [PMC_EI][sc]
    __shared__ int s_end[PMC_EI], s_open;
    const int ii0 = blockIdx.x * PMC_EI, tid = threadIdx.x;
    int wb = sc, we = 0;                                               // the words where any of the block's columns has a row
    for (int e = 0; e < PMC_EI; ++e)
        if (ii0 + e < W) { const int2 r = wr[ii0 + e]; if (r.y > r.x) { wb = min(wb, r.x); we = max(we, r.y); } }
    for (int i = tid; i < PMC_EI * sc; i += 256) {
        const int e = i / sc, w = i - e * sc;
        sL[i] = ii0 + e < W ? LC[(size_t)w * W + ii0 + e] : 0ull;
    }
    if (tid < PMC_EI) s_end[tid] = ii0 + tid < W ? W : -1;             // -1: no such column
    if (tid == 0) s_open = 0;
    __syncthreads();
    for (int base = ii0 + 20; base < W; base += 256) {
        const int jj = base + tid;
        int cnt[PMC_EI];
#pragma unroll
        for (int e = 0; e < PMC_EI; ++e) cnt[e] = 0;
        if (jj < W)
            for (int w = wb; w < we; ++w) {
                const unsigned long long l = LC[(size_t)w * W + jj];
#pragma unroll
                for (int e = 0; e < PMC_EI; ++e) cnt[e] += __popcll(l & sL[e * sc + w]);
            }
#pragma unroll
        for (int e = 0; e < PMC_EI; ++e)
            if (jj < W && jj >= ii0 + e + 20 && cnt[e] < mincov) atomicMin(&s_end[e], jj);
        __syncthreads();
        if (tid == 0) {
            int open = 0;
            for (int e = 0; e < PMC_EI; ++e) if (s_end[e] >= base + 256) open = 1;      // still unbroken beyond this chunk
            s_open = open;
        }
        __syncthreads();
        if (!s_open) break;
    }
    if (tid < PMC_EI && ii0 + tid < W) jend[ii0 + tid] = s_end[tid];
}

// MC:413-434 PositiveSignificance: d_tail_z (hyper_tail.h) and this stage's saturated value.
// `floor`: what the two maxima this pair could raise already hold: a pair that cannot raise either maximum is dropped before
// the sum (after a few thousand partners every variation's maximum is past what chance co-occurrence reaches, and almost
// every pair ends here -- the sums took 93 % of the kernel before).
// The counts k_mc_pairs hands over stay inside what the table covers (hyper_probe_counts_ok states the inequalities): with
// C = LC_i & LC_j (cov rows, cov <= T = the table's reach), gr1 = |G_i & LC_j| and gr2 = |G_j & LC_i| count subsets of C
// because k_mc_bits makes every G a subset of its column's LC; schnitt = |G_i & G_j| is the size of their intersection,
// so schnitt <= min(gr1, gr2) and gr1 + gr2 - schnitt = |union| <= cov; size1 = |G_i| >= gr1, size2 = |G_j| >= gr2.
__device__ __forceinline__ double d_significance(const double *__restrict__ lnf, int schnitt, int cov, int gr1, int gr2, int size1, int size2, double floor)
{
    double Z = d_tail_z(lnf, schnitt, cov, gr1, gr2, floor);
    if (Z > 98.0) Z = 98.0 + 2.0 * schnitt / (2.0 * schnitt + (size1 - schnitt) + (size2 - schnitt));     // F_beta(., ., 1), MC:396-410
    return Z;
}

struct McTile { int jlo, jhi; };    // positions in the list of relevant j this tile of i has to visit: [jlo, jhi)

// grid (tiles of i, chunks of PMC_NT relevant j); Ivar / Jvar = the relevant variations, ascending
__global__ __launch_bounds__(PMC_NT) void k_mc_pairs(int W, int sc, int nI, const int *__restrict__ Ivar, const int *__restrict__ Jvar,
                                                     const McTile *__restrict__ tiles, const unsigned long long *__restrict__ G,
                                                     const unsigned long long *__restrict__ LC, const int *__restrict__ gsize,
                                                     const int *__restrict__ jend, const double *__restrict__ lnf, const int2 *__restrict__ wr,
                                                     unsigned long long *maxc, unsigned long long *npairs)
{
    __shared__ unsigned long long sG[PMC_TI][PMC_WC], sL[PMC_TI][PMC_WC];
    __shared__ int s_i[PMC_TI], s_wb, s_we, s_jb, s_je;
    const McTile tl = tiles[blockIdx.x];
    const int b0 = tl.jlo + blockIdx.y * PMC_NT;
    if (b0 >= tl.jhi) return;
    const int tid = threadIdx.x, a0 = blockIdx.x * PMC_TI;
    if (tid < PMC_TI) s_i[tid] = a0 + tid < nI ? Ivar[a0 + tid] : -1;
    if (tid == 0) { s_wb = sc; s_we = 0; s_jb = sc; s_je = 0; }
    const int b = b0 + tid;
    const bool have = b < tl.jhi;
    const int j = have ? Jvar[b] : 0, jj = j / 5;
    __syncthreads();
    // the words where a row can be in a set of the tile's i AND in a set of the block's j (bit positions follow the rows' first
    // columns, so both are narrow ranges): everything else contributes zero to all four counts
    if (tid < PMC_TI && s_i[tid] >= 0) { const int2 r = wr[s_i[tid] / 5]; if (r.y > r.x) { atomicMin(&s_wb, r.x); atomicMax(&s_we, r.y); } }
    if (have) { const int2 r = wr[jj]; if (r.y > r.x) { atomicMin(&s_jb, r.x); atomicMax(&s_je, r.y); } }
    __syncthreads();
    const int wbeg = max(s_wb, s_jb), wend = min(s_we, s_je), V = W * 5;
    int s[PMC_TI], g1[PMC_TI], g2[PMC_TI], cv[PMC_TI];
#pragma unroll
    for (int a = 0; a < PMC_TI; ++a) s[a] = g1[a] = g2[a] = cv[a] = 0;
    for (int w0 = wbeg; w0 < wend; w0 += PMC_WC) {
        __syncthreads();
        tile_stage<PMC_TI, PMC_WC, PMC_NT>(sG, sL, s_i, G, LC, V, W, w0, wend, tid);
        __syncthreads();
        if (have) tile_count<PMC_TI, PMC_WC>(sG, sL, G, LC, V, W, w0, wend, j, s, g1, g2, cv);
    }
    if (!have) return;
    const int sj = gsize[j];
    const double curj = __longlong_as_double((long long)maxc[j]);
    double zj = 0.0;
    unsigned cnt = 0;
#pragma unroll
    for (int a = 0; a < PMC_TI; ++a) {
        const int i = s_i[a], ii = i / 5;
        if (i >= 0 && jj >= ii + 20 && jj < jend[ii]) {                // MC:798, MC:801-804
            ++cnt;
            const double floor = fmin(fmax(curj, zj), __longlong_as_double((long long)maxc[i]));
            double Z = d_significance(lnf, s[a], cv[a], g1[a], g2[a], gsize[i], sj, floor);
            if (!(Z > 0.0)) Z = 0.0;                                   // (-log10(1) is -0.0, whose bit pattern is the largest of all)
            zj = fmax(zj, Z);
            const unsigned long long zb = (unsigned long long)__double_as_longlong(Z);   // Z >= 0: the bit patterns order like the values
            if (zb > maxc[i]) atomicMax(&maxc[i], zb);                 // MC:816
        }
    }
    const unsigned long long zb = (unsigned long long)__double_as_longlong(zj);
    if (zb > maxc[j]) atomicMax(&maxc[j], zb);                         // MC:817
    if (cnt) atomicAdd(npairs, (unsigned long long)cnt);
}

extern "C" int pmc_last_timing(double *ms5)
{
    if (!ms5) return PWR_ERR_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = g_ms[i];
    return PWR_OK;
}

static int maxcorrs_on_device(int T, int W, const unsigned char *text, int mincov, int device, double *maxcorrs)
{
    if (T <= 0 || W <= 0 || !text || !maxcorrs || mincov < 0) return PWR_ERR_ARG;
    if (T > PMC_MAX_ROWS || W > PMC_MAX_COLUMNS) return PWR_ERR_RANGE;
    if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
    const double t0 = now_ms();
    const int sc = T / 64 + 1;                                                       // MC:338
    const size_t nv = (size_t)W * 5;
    typedef unsigned long long u64;
    DevArena dev;
    unsigned char *d_text = dev.put(text, (size_t)T * W);
    u64 *d_G = dev.get<u64>(nv * sc), *d_LC = dev.get<u64>((size_t)W * sc), *d_maxc = dev.get<u64>(nv), *d_npairs = dev.get<u64>(1);
    int *d_gsize = dev.get<int>(nv), *d_cover = dev.get<int>(W), *d_jend = dev.get<int>(W), *d_start = dev.get<int>(T), *d_inv = dev.get<int>(T);
    int2 *d_wr = dev.get<int2>(W);
    if (!d_text || !d_G || !d_LC || !d_maxc || !d_npairs || !d_gsize || !d_cover || !d_jend || !d_start || !d_inv || !d_wr) return dev.err;
    HIPC(hipMemset(d_gsize, 0, nv * 4)); HIPC(hipMemset(d_cover, 0, (size_t)W * 4)); HIPC(hipMemset(d_maxc, 0, nv * 8)); HIPC(hipMemset(d_npairs, 0, 8));
    // bit positions in the order of the rows' first covered columns
    hipLaunchKernelGGL(k_mc_rowstart, dim3(T), dim3(256), 0, 0, W, d_text, d_start);
    HIPC(hipGetLastError());
    std::vector<int> start(T), inv(T);
    HIPC(hipMemcpy(start.data(), d_start, (size_t)T * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < T; ++r) inv[r] = r;
    std::stable_sort(inv.begin(), inv.end(), [&](int a, int b) { return start[a] < start[b]; });
    HIPC(hipMemcpy(d_inv, inv.data(), (size_t)T * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mc_bits, dim3((W + 255) / 256, sc), dim3(256), 0, 0, T, W, sc, d_text, d_inv, d_G, d_LC, d_gsize, d_cover);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_mc_colrange, dim3((W + 255) / 256), dim3(256), 0, 0, W, sc, d_LC, d_wr);
    HIPC(hipGetLastError());
    std::vector<int> gsize(nv), cover(W), jend(W);
    HIPC(hipMemcpy(gsize.data(), d_gsize, nv * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(cover.data(), d_cover, (size_t)W * 4, hipMemcpyDeviceToHost));
    const double t1 = now_ms();
    const size_t lds_end = (size_t)PMC_EI * sc * 8;
    hipLaunchKernelGGL(k_mc_end, dim3((W + PMC_EI - 1) / PMC_EI), dim3(256), lds_end, 0, W, sc, mincov, d_LC, d_wr, d_jend);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(jend.data(), d_jend, (size_t)W * 4, hipMemcpyDeviceToHost));
    const double t2 = now_ms();
    // the relevant variations (MC:796, MC:811): i needs more than mincov / 4 and fewer than all rows, and bases in more than
    // half of its column's covered rows; j only the first two
    const int maxgroup = T;                                                           // MC:1007
    std::vector<int> Ivar, Jvar;
    for (int c = 0; c < W; ++c) {
        const int baseno = gsize[c * 5] + gsize[c * 5 + 1] + gsize[c * 5 + 2] + gsize[c * 5 + 3];
        for (int k = 0; k < 5; ++k) {
            const int v = c * 5 + k;
            if (gsize[v] > mincov / 4 && gsize[v] < maxgroup) {
                Jvar.push_back(v);
                if (baseno > cover[c] / 2) Ivar.push_back(v);
            }
        }
    }
    const int nI = (int)Ivar.size(), nJ = (int)Jvar.size();
    unsigned long long npairs = 0;
    if (nI && nJ) {
        const int ntiles = (nI + PMC_TI - 1) / PMC_TI;
        std::vector<McTile> tiles(ntiles);
        int maxspan = 0;
        for (int t = 0; t < ntiles; ++t) {
            int clo = W, chi = 0;                                                     // columns any i of the tile visits
            for (int a = t * PMC_TI; a < std::min(nI, (t + 1) * PMC_TI); ++a) {
                const int ii = Ivar[a] / 5;
                clo = std::min(clo, ii + 20); chi = std::max(chi, jend[ii]);
            }
            const int jlo = (int)(std::lower_bound(Jvar.begin(), Jvar.end(), clo * 5) - Jvar.begin());
            const int jhi = (int)(std::lower_bound(Jvar.begin(), Jvar.end(), chi * 5) - Jvar.begin());
            tiles[t].jlo = jlo; tiles[t].jhi = std::max(jlo, jhi);
            maxspan = std::max(maxspan, tiles[t].jhi - tiles[t].jlo);
        }
        if (maxspan > 0) {
            const std::vector<double> lnf = hyper_lnf_table(T);
            const int *d_Ivar = dev.put(Ivar.data(), nI), *d_Jvar = dev.put(Jvar.data(), nJ);
            const McTile *d_tiles = dev.put(tiles.data(), ntiles);
            const double *d_lnf = dev.put(lnf.data(), lnf.size());
            if (!d_Ivar || !d_Jvar || !d_tiles || !d_lnf) return dev.err;
            hipLaunchKernelGGL(k_mc_pairs, dim3(ntiles, (maxspan + PMC_NT - 1) / PMC_NT), dim3(PMC_NT), 0, 0, W, sc, nI, d_Ivar, d_Jvar, d_tiles,
                               d_G, d_LC, d_gsize, d_jend, d_lnf, d_wr, d_maxc, d_npairs);
            HIPC(hipGetLastError());
        }
    }
    HIPC(hipMemcpy(maxcorrs, d_maxc, nv * 8, hipMemcpyDeviceToHost));                 // (bit patterns of non-negative doubles)
    HIPC(hipMemcpy(&npairs, d_npairs, 8, hipMemcpyDeviceToHost));
    const double t3 = now_ms();
    g_ms[0] = t3 - t0; g_ms[1] = t1 - t0; g_ms[2] = t2 - t1; g_ms[3] = t3 - t2; g_ms[4] = (double)npairs;
    return PWR_OK;
}

extern "C" int pmc_maxcorrs(int T, int W, const unsigned char *text, int mincov, int device, double *maxcorrs)
{
    return abi_guard([&] { return maxcorrs_on_device(T, W, text, mincov, device, maxcorrs); });
}

// ---- test hook: the tail functions k_mc_pairs calls, as this file compiles them, on given counts (thread = one tuple) ----
__global__ __launch_bounds__(256) void k_mc_tail_probe(int n, const int *__restrict__ counts, const double *__restrict__ floor,
                                                       const double *__restrict__ lnf, double *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int *c = counts + (size_t)t * 6;
    const int s = c[0], cov = c[1], g1 = c[2], g2 = c[3];
    const double fl = floor ? floor[t] : 0.0;
    double *o = out + (size_t)t * 4;
    o[0] = d_hyper_Q(lnf, (unsigned)(s - 1), (unsigned)g2, (unsigned)(cov - g2), (unsigned)g1);
    o[1] = d_tail_z(lnf, s, cov, g1, g2, 0.0);
    o[2] = d_tail_z(lnf, s, cov, g1, g2, fl);
    o[3] = d_significance(lnf, s, cov, g1, g2, c[4], c[5], fl);
}

extern "C" int pmc_tail_probe(int n, const int *counts, const double *floor, int device, double *out)
{
    return abi_guard([&] {
        return hyper_probe_run(n, counts, floor, device, PMC_MAX_ROWS, 4, out, [](int m, const int *c, const double *f, const double *l, double *o) {
            hipLaunchKernelGGL(k_mc_tail_probe, dim3((m + 255) / 256), dim3(256), 0, 0, m, c, f, l, o);
        });
    });
}
