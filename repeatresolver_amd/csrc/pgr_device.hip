// pgr_device.hip -- MI355X (gfx950) implementation of RepeatResolver's group refinement behind include/pgr.h.
//
// Reference: PhilippBongartz/RepeatResolver, RepeatResolver.c ("RR:"), Group_Refinement (RR:1634-1690): for every variation a
// whose MaxCorrs exceed the cutoff, Cliquer (RR:1179-1240) scans every variation i of the window, scores the pair with four
// sizes of intersections of row bit sets and one upper tail of a hypergeometric distribution (RR:472-488) and keeps the 29
// best; the clique's row sets are then voted into a refined group and its coverage (RR:1460-1522, RR:976-1008, RR:1064-1096).
//   k_gr_cliques  a tiled bit-set product like k_mc_pairs: a tile of PGR_TA significant a stays in LDS (their group and their
//                 column's coverage, a chunk of words at a time), every thread owns one variation i per chunk of PGR_NT and
//                 streams its two bit sets once.  A block walks a slice of the chunks and keeps, per a, the best 29 of its
//                 slice in LDS; the running 29th value is the floor of the tail's early-out.
//   k_gr_votes    one work-group per significant a: merges the slices' lists into the clique, then Sizes, the vote
//                 histogram, Dropoff_Cutoff, and the refined group / coverage, one wave ballot per 64-row word.
//   k_gr_reldrop  RelativeDropoff_Subdivision (RR:3274-3378): one work-group per selected variation, its rows' votes
//                 scattered into per-partition histograms in LDS; behind pgr_subdivide at the end of this file.
// TheBestUpdater (RR:1156-1176) never displaces on equality and inserts behind equal values, and the scan ascends in i: the
// clique is the top 29 by (Z descending, i ascending), whatever the order of evaluation.  `better` below is that key.
// This file is compiled with -ffp-contract=off: the saturated value 97.90 + F must be one division and one addition, so
// that equal fractions give equal doubles here and on any host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PWR_STAGE "pgr"
#include "dev_util.h"
#include "four_count_tile.h"
#include "hyper_tail.h"
#include "pgr.h"
#include "pgr_internal.h"

#define PGR_TA 16                   // significant variations a per tile
#define PGR_NT 256                  // threads per block = variations i per chunk
#define PGR_WC 32                   // words per LDS chunk
#define PGR_KEEP (PGR_MAXCLIQUE - 1) // partners kept per a
#define PGR_MAXSLICES 16            // slices of the i range (partial lists per a)

static double g_ms[5] = {0, 0, 0, 0, 0};

// (z1, i1) ranks before (z2, i2)
__device__ __forceinline__ bool better(double z1, int i1, double z2, int i2)
{
    return z1 > z2 || (z1 == z2 && i1 < i2);
}

// RR:472-488 Group_PositiveSignificance(G_i, G_a, LC_i, LC_a) from the four counts and the two group sizes: d_tail_z
// (hyper_tail.h) and this stage's saturated value.  `floor`: what a value has to reach to matter (greedy, or the 29th of
// the running list).
// The counts k_gr_cliques hands over stay inside what the table covers (hyper_probe_counts_ok states the inequalities): the
// window reader sets a row's bit in a group and in its column's coverage together, so every G is a subset of its LC; with
// C = LC_i & LC_a (cov rows, cov <= kept rows = the table's reach), gr1 = |G_i & LC_a| and gr2 = |G_a & LC_i| count
// subsets of C whose intersection is G_i & G_a: schnitt <= min(gr1, gr2), gr1 + gr2 - schnitt = |union| <= cov; the sizes
// are |G_i| >= gr1 and |G_a| >= gr2 (gsize is the popcount of the same sets).
__device__ __forceinline__ double d_gr_significance(const double *__restrict__ lnf, int schnitt, int cov, int gr1, int gr2, int size_i, int size_a, double floor)
{
    double Z = d_tail_z(lnf, schnitt, cov, gr1, gr2, floor);                                   // RR:451-453
    if (Z > 98.0) Z = 97.90 + (double)(2 * schnitt) / (double)(size_i + size_a);   // F_beta(., ., 1), RR:432-447: 2s + |i \ a| + |a \ i|
    return Z;
}

// grid (tiles of a, slices of the i range); Svar = the significant variations, ascending; G[w][v], LC[w][column]
__global__ __launch_bounds__(PGR_NT) void k_gr_cliques(int V, int W, int sc, int nS, const int *__restrict__ Svar,
                                                       const unsigned long long *__restrict__ G, const unsigned long long *__restrict__ LC,
                                                       const int *__restrict__ gsize, const double *__restrict__ lnf, int mincov4, double greedy,
                                                       int cps, int nslices, double *__restrict__ pZ, int *__restrict__ pI)
{
    __shared__ unsigned long long sG[PGR_TA][PGR_WC], sL[PGR_TA][PGR_WC];
    __shared__ double lZ[PGR_TA][32], cZ[PGR_NT];
    __shared__ int lI[PGR_TA][32], lN[PGR_TA], cI[PGR_NT], s_cnt[PGR_TA], s_a[PGR_TA];
    const int tid = threadIdx.x, a0 = blockIdx.x * PGR_TA, slice = blockIdx.y;
    if (tid < PGR_TA) { s_a[tid] = a0 + tid < nS ? Svar[a0 + tid] : -1; lN[tid] = 0; }
    const int nch = (V + PGR_NT - 1) / PGR_NT, ch0 = slice * cps, ch1 = min(nch, ch0 + cps);
    for (int ch = ch0; ch < ch1; ++ch) {
        const int i = ch * PGR_NT + tid;
        const bool have = i < V;
        int s[PGR_TA], g1[PGR_TA], g2[PGR_TA], cv[PGR_TA];
#pragma unroll
        for (int a = 0; a < PGR_TA; ++a) s[a] = g1[a] = g2[a] = cv[a] = 0;
        for (int w0 = 0; w0 < sc; w0 += PGR_WC) {
            __syncthreads();                                           // (everyone is done with the chunk before)
            if (w0 == 0 && tid < PGR_TA) s_cnt[tid] = 0;
            tile_stage<PGR_TA, PGR_WC, PGR_NT>(sG, sL, s_a, G, LC, V, W, w0, sc, tid);
            __syncthreads();
            if (have) tile_count<PGR_TA, PGR_WC>(sG, sL, G, LC, V, W, w0, sc, i, s, g2, g1, cv);   // g1 = |G_i & LC_a|, g2 = |G_a & LC_i|
        }
        const int si = have ? gsize[i] : 0;
#pragma unroll
        for (int a = 0; a < PGR_TA; ++a) {
            const int va = s_a[a];                                     // (the same for the whole block, as is every branch with a barrier)
            if (va < 0) continue;
            const int n = lN[a];
            const double lastZ = n == PGR_KEEP ? lZ[a][PGR_KEEP - 1] : greedy;
            const int lastI = n == PGR_KEEP ? lI[a][PGR_KEEP - 1] : -1;
            double Z = 0.0;
            if (have && i != va && s[a] > mincov4)                     // RR:1209, RR:1214
                Z = d_gr_significance(lnf, s[a], cv[a], g1[a], g2[a], si, gsize[va], lastZ);
            if (Z > greedy && (n < PGR_KEEP || better(Z, i, lastZ, lastI))) {      // RR:1217, RR:1158
                const int slot = atomicAdd(&s_cnt[a], 1);              // (at most one per thread: slot < PGR_NT)
                cZ[slot] = Z; cI[slot] = i;
            }
            __syncthreads();
            const int cnt = s_cnt[a];
            if (cnt == 0) continue;
            // the new list = the best PGR_KEEP of list + candidates: everyone finds the rank of its entry among all of them
            int rc = -1, rl = -1, myI = 0, eI = 0;
            double myZ = 0.0, eZ = 0.0;
            if (tid < cnt) {
                myZ = cZ[tid]; myI = cI[tid]; rc = 0;
                for (int t = 0; t < n; ++t) rc += better(lZ[a][t], lI[a][t], myZ, myI);
                for (int t = 0; t < cnt; ++t) rc += better(cZ[t], cI[t], myZ, myI);
            }
            if (tid < n) {
                eZ = lZ[a][tid]; eI = lI[a][tid]; rl = tid;
                for (int t = 0; t < cnt; ++t) rl += better(cZ[t], cI[t], eZ, eI);
            }
            __syncthreads();
            if (rc >= 0 && rc < PGR_KEEP) { lZ[a][rc] = myZ; lI[a][rc] = myI; }
            if (rl >= 0 && rl < PGR_KEEP) { lZ[a][rl] = eZ; lI[a][rl] = eI; }
            if (tid == 0) lN[a] = min(PGR_KEEP, n + cnt);
            __syncthreads();
        }
    }
    __syncthreads();
    for (int t = tid; t < PGR_TA * PGR_KEEP; t += PGR_NT) {
        const int a = t / PGR_KEEP, k = t - a * PGR_KEEP;
        if (s_a[a] < 0) continue;
        const size_t o = ((size_t)(a0 + a) * nslices + slice) * PGR_KEEP + k;
        const bool ok = k < lN[a];
        pZ[o] = ok ? lZ[a][k] : 0.0;
        pI[o] = ok ? lI[a][k] : -1;
    }
}

// block = one significant variation
__global__ __launch_bounds__(256) void k_gr_votes(int V, int W, int sc, int nk, int nslices, const int *__restrict__ Svar,
                                                  const double *__restrict__ pZ, const int *__restrict__ pI,
                                                  const unsigned long long *__restrict__ G, const unsigned long long *__restrict__ LC,
                                                  int *__restrict__ cliques, int *__restrict__ sizes, int *__restrict__ cutoffs, double *__restrict__ drop_off,
                                                  unsigned long long *__restrict__ cg, unsigned long long *__restrict__ cc)
{
    __shared__ double mZ[PGR_MAXSLICES * PGR_KEEP];
    __shared__ int mI[PGR_MAXSLICES * PGR_KEEP], s_clique[PGR_MAXCLIQUE + 1], s_hist[32], s_sizes, s_nall, s_cut;
    const int sidx = blockIdx.x, tid = threadIdx.x, a = Svar[sidx], tot = nslices * PGR_KEEP;
    for (int t = tid; t < tot; t += 256) { mZ[t] = pZ[(size_t)sidx * tot + t]; mI[t] = pI[(size_t)sidx * tot + t]; }
    if (tid <= PGR_MAXCLIQUE) s_clique[tid] = tid == 0 ? a : -1;      // RR:1196; unfilled slots and Clique[30] are -1 (RR:1229-1231)
    if (tid < 32) s_hist[tid] = 0;
    __syncthreads();
    for (int t = tid; t < tot; t += 256) {
        if (mI[t] < 0) continue;
        int r = 0;
        for (int u = 0; u < tot; ++u) r += mI[u] >= 0 && better(mZ[u], mI[u], mZ[t], mI[t]);
        if (r < PGR_KEEP) s_clique[1 + r] = mI[t];
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0, nall = 0;
        while (s_clique[n] > 0) n++;                                   // RR:1650: variation 0 as a member ends the count
        while (s_clique[nall] >= 0) nall++;                            // RR:982-989
        s_sizes = n; s_nall = nall;
        sizes[sidx] = n;
    }
    if (tid <= PGR_MAXCLIQUE) cliques[(size_t)sidx * (PGR_MAXCLIQUE + 1) + tid] = s_clique[tid];
    __syncthreads();
    const int n = s_sizes, nall = s_nall;
    if (n <= 5) {                                                      // RR:1684-1687 (the host zeroes MaxCorrs[a])
        if (tid == 0) { cutoffs[sidx] = 0; drop_off[sidx] = 1000.0; }
        return;
    }
    const int wave = tid >> 6, lane = tid & 63;
    for (int w = wave; w < sc; w += 4) {                               // RR:1471-1482: in how many of the first Sizes groups is the row
        int v = 0;
        for (int m = 0; m < n; ++m) v += (int)((G[(size_t)w * V + s_clique[m]] >> lane) & 1ull);
        if (w * 64 + lane < nk && v > 0) atomicAdd(&s_hist[v], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int sz[PGR_MAXCLIQUE + 2];                                     // sizes[k] = rows in more than k groups
        int run = 0;
        for (int k = PGR_MAXCLIQUE; k >= 0; --k) { run += k + 1 < 32 ? s_hist[k + 1] : 0; sz[k] = run; }
        int c = 1;                                                     // RR:1487-1508
        double min_drop = 1000000.0;
        for (int k = 1; k < n - 1; ++k) {
            const int m = min(nk - sz[k], sz[k]);
            if (m > 0) {
                const double drop = (double)(sz[k - 1] - sz[k + 1]) / (double)m;
                if (drop < min_drop) { min_drop = drop; c = k; }
            }
        }
        s_cut = c;
        cutoffs[sidx] = c; drop_off[sidx] = min_drop;
    }
    __syncthreads();
    const int c = s_cut;
    for (int w = wave; w < sc; w += 4) {                               // RR:991-1006, RR:1079-1094: over ALL members
        int vg = 0, vc = 0;
        for (int m = 0; m < nall; ++m) {
            const int mem = s_clique[m];
            vg += (int)((G[(size_t)w * V + mem] >> lane) & 1ull);
            vc += (int)((LC[(size_t)w * W + mem / 5] >> lane) & 1ull);
        }
        const bool in = w * 64 + lane < nk;
        const unsigned long long bg = __ballot(in && vg > c), bc = __ballot(in && vc > c);
        if (lane == 0) { cg[(size_t)sidx * sc + w] = bg; cc[(size_t)sidx * sc + w] = bc; }
    }
}

// RelativeDropoff_Subdivision (RR:3274-3378), every (partition k, selected variation) pair in one pass.  Block = one selected
// variation; a lane per row as in k_gr_votes.  A row's two vote counts do not depend on k (RR:2873-2880 over the first
// Sizes members, RR:982-1001 over all of them), so they are computed once per row and scattered into the histograms of
// the row's partition in LDS, keyed by lab[] (the index among the partitions with more than 2 * mingroup rows, -1: skip).
// One word per (partition, vote count): the low half counts v_sizes, the high half v_all; a partition has at most nk <
// 65536 rows (checked by the host), so no half carries into the other.  PGR_SD_TILE partitions per pass, as many passes
// as E needs.  Per partition one thread then runs the drop loop of RR:2896-2908 in double and counts drinne / draus; a
// (variation, c) that would split competes with an atomic minimum on (rank in the selected list) << 5 | c: the first split
// of a partition is the only one.
#define PGR_SD_TILE 64
#define PGR_SD_STRIDE 33            // words per partition in LDS: odd, so the evaluating threads hit different banks

__global__ __launch_bounds__(256) void k_gr_reldrop(int Vc, int sc, int nk, int E, int mingroup, const int *__restrict__ selcl,
                                                    const int *__restrict__ selsz, const int *__restrict__ lab,
                                                    const unsigned long long *__restrict__ G, unsigned int *__restrict__ best)
{
    __shared__ unsigned int s_h[PGR_SD_TILE * PGR_SD_STRIDE];
    __shared__ int s_clique[PGR_MAXCLIQUE + 2], s_nall;
    const int sidx = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid <= PGR_MAXCLIQUE) s_clique[tid] = selcl[(size_t)sidx * (PGR_MAXCLIQUE + 1) + tid];
    __syncthreads();
    if (tid == 0) {
        int nall = 0;
        while (nall < PGR_MAXCLIQUE && s_clique[nall] >= 0) nall++;   // RR:982-989 (the host checked the members)
        s_nall = nall;
    }
    __syncthreads();
    const int n = selsz[sidx], nall = s_nall;                          // Sizes <= nall <= 30
    for (int p0 = 0; p0 < E; p0 += PGR_SD_TILE) {
        const int np = min(PGR_SD_TILE, E - p0);
        for (int t = tid; t < np * PGR_SD_STRIDE; t += 256) s_h[t] = 0u;
        __syncthreads();
        for (int w = wave; w < sc; w += 4) {
            const int e = lab[w * 64 + lane] - p0;                     // lab[sc * 64], -1 beyond nk
            const bool mine = e >= 0 && e < np;
            if (__ballot(mine) == 0ull) continue;                      // no row of this word in this pass (the same for the wave)
            int vs = 0, va = 0;
            for (int m = 0; m < nall; ++m) {
                const int b = (int)((G[(size_t)w * Vc + s_clique[m]] >> lane) & 1ull);
                va += b;
                vs += m < n ? b : 0;
            }
            if (mine) {
                unsigned int *h = s_h + e * PGR_SD_STRIDE;
                if (vs == va) atomicAdd(h + vs, 0x10001u);
                else { atomicAdd(h + vs, 1u); atomicAdd(h + va, 0x10000u); }
            }
        }
        __syncthreads();
        if (tid < np) {
            unsigned int h[32];
            int sz[32];                                                // sizes[k] = rows of the partition in more than k groups
#pragma unroll
            for (int k = 0; k < 32; ++k) h[k] = s_h[tid * PGR_SD_STRIDE + k];
            int run = 0;
#pragma unroll
            for (int k = 31; k >= 0; --k) { sz[k] = run; run += (int)(h[k] & 0xffffu); }
            const int count = run;
            int c = 1;                                                 // RR:2886-2908 with c = 0
            double min_drop = 1000000.0;
#pragma unroll
            for (int i = 1; i < PGR_MAXCLIQUE - 1; ++i) {
                if (i < n - 1) {
                    const int m = min(nk - sz[i], sz[i]);              // RR:2898: signumber, not the partition's size
                    if (m > 0) {
                        const double drop = (double)(sz[i - 1] - sz[i + 1]) / (double)m;
                        if (drop < min_drop) { min_drop = drop; c = i; }
                    }
                }
            }
            if (min_drop < 0.0001) {                                   // RR:3336
                int drinne = 0;                                        // rows of the partition in CliqueGroup(Clique, c)
#pragma unroll
                for (int k = 0; k < 32; ++k) drinne += k > c ? (int)(h[k] >> 16) : 0;
                const int draus = count - drinne;
                if (drinne > mingroup && draus > mingroup) atomicMin(&best[p0 + tid], ((unsigned int)sidx << 5) | (unsigned int)c);
            }
        }
        __syncthreads();
    }
}

struct WindowGuard {
    pgr_window w;
    WindowGuard() { memset(&w, 0, sizeof w); }
    ~WindowGuard() { pgr_window_free(&w); }
};

extern "C" int pgr_last_timing(double *ms5)
{
    if (!ms5) return PWR_ERR_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = g_ms[i];
    return PWR_OK;
}

extern "C" void pgr_free(pgr_result *r)
{
    if (!r) return;
    free(r->kept); free(r->maxcorrs); free(r->significant); free(r->sizes); free(r->cliques); free(r->cutoffs); free(r->drop_off);
    free(r->c_groups); free(r->c_coverage);
    memset(r, 0, sizeof *r);
}

// The host part in front of the kernels (RR:3977-4014, RR:1647): the MaxCorrs slice, the cutoff, the coverage restriction, the
// significant variations, and res's arrays (zeroed).
static int refine_prepare(int rows, int nk, int W, int sc, int von, int bis, const unsigned char *kept, const int *coverage,
                          const double *maxcorrs_full, int msa_width, double *cutoff, pgr_result *res, std::vector<int> &Svar)
{
    const size_t V = (size_t)W * 5;
    res->rows = rows; res->kept_rows = nk; res->width = W; res->sc = sc;
    res->kept = (unsigned char *)malloc((size_t)rows);
    res->maxcorrs = (double *)malloc(sizeof(double) * V);
    if (!res->kept || !res->maxcorrs) return PWR_ERR_NOMEM;
    memcpy(res->kept, kept, (size_t)rows);
    int rc;
    if ((rc = pgr_slice_maxcorrs(maxcorrs_full, msa_width * 5, von, bis, res->maxcorrs))) return rc;
    *cutoff = pgr_default_cutoff(*cutoff, W);
    res->cutoff = *cutoff;
    if ((rc = pgr_restrict_coverage(W, coverage, res->maxcorrs, nullptr))) return rc;
    for (size_t i = 0; i < V; ++i) if (res->maxcorrs[i] > *cutoff) Svar.push_back((int)i);         // RR:1647
    const int nS = (int)Svar.size();
    res->nsig = nS;
    const size_t n1 = nS ? nS : 1;
    res->significant = (int *)calloc(n1, sizeof(int)); res->sizes = (int *)calloc(n1, sizeof(int));
    res->cliques = (int *)calloc(n1 * (PGR_MAXCLIQUE + 1), sizeof(int)); res->cutoffs = (int *)calloc(n1, sizeof(int));
    res->drop_off = (double *)calloc(n1, sizeof(double));
    res->c_groups = (unsigned long long *)calloc(n1 * sc, 8); res->c_coverage = (unsigned long long *)calloc(n1 * sc, 8);
    if (!res->significant || !res->sizes || !res->cliques || !res->cutoffs || !res->drop_off || !res->c_groups || !res->c_coverage) return PWR_ERR_NOMEM;
    if (nS) memcpy(res->significant, Svar.data(), sizeof(int) * nS);
    return PWR_OK;
}

// The kernels, on sets that are on the device (the current one): fills res's arrays; ms2: cliques, votes
static int refine_on_device(const unsigned long long *dG, const unsigned long long *dLC, const int *dgsize, int nk, int W, int sc,
                            const std::vector<int> &Svar, int mincov, double cutoff, pgr_result *res, double *ms2)
{
    const size_t V = (size_t)W * 5;
    const int nS = (int)Svar.size();
    const std::vector<double> lnf = hyper_lnf_table(nk);
    const int nch = (int)((V + PGR_NT - 1) / PGR_NT), ntiles = (nS + PGR_TA - 1) / PGR_TA;
    // enough blocks to fill the device when there are few tiles of a, long slices (a better floor) when there are many
    int want = std::max(1, std::min(PGR_MAXSLICES, (2048 + ntiles - 1) / ntiles));
    want = std::min(want, nch);
    const int cps = (nch + want - 1) / want, nslices = (nch + cps - 1) / cps;
    typedef unsigned long long u64;
    DevArena dev;
    const size_t np = (size_t)nS * nslices * PGR_KEEP;
    const int *d_Svar = dev.put(Svar.data(), nS);
    const double *d_lnf = dev.put(lnf.data(), lnf.size());
    double *d_pZ = dev.get<double>(np), *d_drop = dev.get<double>(nS);
    int *d_pI = dev.get<int>(np), *d_cliques = dev.get<int>((size_t)nS * (PGR_MAXCLIQUE + 1)), *d_sizes = dev.get<int>(nS), *d_cutoffs = dev.get<int>(nS);
    u64 *d_cg = dev.get<u64>((size_t)nS * sc), *d_cc = dev.get<u64>((size_t)nS * sc);
    if (!d_Svar || !d_lnf || !d_pZ || !d_drop || !d_pI || !d_cliques || !d_sizes || !d_cutoffs || !d_cg || !d_cc) return dev.err;
    HIPC(hipMemset(d_cg, 0, (size_t)nS * sc * 8)); HIPC(hipMemset(d_cc, 0, (size_t)nS * sc * 8));
    HIPC(hipDeviceSynchronize());
    const double t1 = now_ms();
    hipLaunchKernelGGL(k_gr_cliques, dim3(ntiles, nslices), dim3(PGR_NT), 0, 0, (int)V, W, sc, nS, d_Svar, dG, dLC, dgsize, d_lnf, mincov / 4, cutoff,
                       cps, nslices, d_pZ, d_pI);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    const double t2 = now_ms();
    hipLaunchKernelGGL(k_gr_votes, dim3(nS), dim3(256), 0, 0, (int)V, W, sc, nk, nslices, d_Svar, d_pZ, d_pI, dG, dLC, d_cliques, d_sizes, d_cutoffs,
                       d_drop, d_cg, d_cc);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(res->cliques, d_cliques, (size_t)nS * (PGR_MAXCLIQUE + 1) * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(res->sizes, d_sizes, (size_t)nS * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(res->cutoffs, d_cutoffs, (size_t)nS * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(res->drop_off, d_drop, (size_t)nS * 8, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(res->c_groups, d_cg, (size_t)nS * sc * 8, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(res->c_coverage, d_cc, (size_t)nS * sc * 8, hipMemcpyDeviceToHost));
    for (int s = 0; s < nS; ++s)
        if (res->sizes[s] <= 5) res->maxcorrs[Svar[s]] = 0.0;                                    // RR:1686
    ms2[0] = t2 - t1; ms2[1] = now_ms() - t2;
    return PWR_OK;
}

static int refine(int rows, int width, const unsigned char *text, const double *maxcorrs_full, int von, int bis, int mincov, double cutoff,
                  int device, pgr_result *res)
{
    const double t0 = now_ms();
    WindowGuard wg;
    int rc = pgr_read_window(rows, width, text, von, bis, &wg.w);
    if (rc) return rc;
    const pgr_window &win = wg.w;
    const int W = win.width, sc = win.sc, nk = win.kept_rows;
    const size_t V = (size_t)W * 5;
    std::vector<int> Svar;
    if ((rc = refine_prepare(rows, nk, W, sc, win.von, win.bis, win.kept, win.coverage, maxcorrs_full, width, &cutoff, res, Svar))) return rc;
    const int nS = (int)Svar.size();
    g_ms[1] = g_ms[2] = g_ms[3] = g_ms[4] = 0;
    if (nS == 0) { g_ms[0] = now_ms() - t0; return PWR_OK; }
    if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
    // word-major copies for the device: the threads of a wave read neighbouring variations of one word
    std::vector<unsigned long long> Gt(V * sc), Lt((size_t)W * sc);
    std::vector<int> gsize(V, 0);
    pgr_word_major(win.groups, sc, nullptr, V, Gt.data());
    pgr_word_major(win.local_coverage, sc, nullptr, (size_t)W, Lt.data());
    for (size_t v = 0; v < V; ++v)
        for (int w = 0; w < sc; ++w) gsize[v] += __builtin_popcountll(win.groups[v * sc + w]);
    DevArena sets;                                                     // the sets of this call's own window
    const unsigned long long *dG = sets.put(Gt.data(), Gt.size()), *dLC = sets.put(Lt.data(), Lt.size());
    const int *dgsize = sets.put(gsize.data(), V);
    if (!dG || !dLC || !dgsize) return sets.err;
    double ms2[2] = {0, 0};
    if ((rc = refine_on_device(dG, dLC, dgsize, nk, W, sc, Svar, mincov, cutoff, res, ms2))) return rc;
    const double t3 = now_ms();
    g_ms[0] = t3 - t0; g_ms[2] = ms2[0]; g_ms[3] = ms2[1]; g_ms[1] = g_ms[0] - ms2[0] - ms2[1]; g_ms[4] = (double)nS * (double)(V - 1);
    return PWR_OK;
}

extern "C" int pgr_refine(int rows, int width, const unsigned char *text, const double *maxcorrs_full, int von, int bis, int mincov, double cutoff,
                          int device, pgr_result *result)
{
    if (!result) return PWR_ERR_ARG;
    memset(result, 0, sizeof *result);
    if (rows <= 0 || width <= 0 || !text || !maxcorrs_full || mincov < 0) return PWR_ERR_ARG;
    if (!(cutoff <= 100.0)) return PWR_ERR_ARG;                        // the trim of RR:1228-1231 needs greedy <= Best_Corrs[0] = 100
    const int rc = abi_guard([&] { return refine(rows, width, text, maxcorrs_full, von, bis, mincov, cutoff, device, result); });
    if (rc) pgr_free(result);
    return rc;
}

int pgr_refine_sets(const pgr_device_sets *sets, const unsigned char *kept, const int *coverage, const double *maxcorrs_full, int msa_width,
                    int mincov, double cutoff, int device, pgr_result *result, double *ms2)
{
    if (!result) return PWR_ERR_ARG;
    memset(result, 0, sizeof *result);
    if (ms2) ms2[0] = ms2[1] = 0;
    if (!sets || !kept || !coverage || !maxcorrs_full || mincov < 0 || !sets->G || !sets->LC || !sets->gsize) return PWR_ERR_ARG;
    if (!(cutoff <= 100.0)) return PWR_ERR_ARG;
    double ms[2] = {0, 0};
    const int rc = abi_guard([&] {
        std::vector<int> Svar;
        const int rp = refine_prepare(sets->rows, sets->kept_rows, sets->width, sets->sc, sets->von, sets->bis, kept, coverage, maxcorrs_full,
                                      msa_width, &cutoff, result, Svar);
        if (rp || Svar.empty()) return rp;
        if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
        return refine_on_device(sets->G, sets->LC, sets->gsize, sets->kept_rows, sets->width, sets->sc, Svar, mincov, cutoff, result, ms);
    });
    if (rc) { pgr_free(result); return rc; }
    if (ms2) { ms2[0] = ms[0]; ms2[1] = ms[1]; }
    return PWR_OK;
}

// ---- test hook: the tail functions k_gr_cliques calls, as this file compiles them, on given counts (thread = one tuple) ----
__global__ __launch_bounds__(256) void k_gr_tail_probe(int n, const int *__restrict__ counts, const double *__restrict__ floor,
                                                       const double *__restrict__ lnf, double *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int *c = counts + (size_t)t * 6;
    const double fl = floor ? floor[t] : 0.0;
    out[(size_t)t * 2] = d_tail_z(lnf, c[0], c[1], c[2], c[3], fl);
    out[(size_t)t * 2 + 1] = d_gr_significance(lnf, c[0], c[1], c[2], c[3], c[4], c[5], fl);
}

extern "C" int pgr_tail_probe(int n, const int *counts, const double *floor, int device, double *out)
{
    return abi_guard([&] {
        return hyper_probe_run(n, counts, floor, device, PGR_MAX_ROWS, 2, out, [](int m, const int *c, const double *f, const double *l, double *o) {
            hipLaunchKernelGGL(k_gr_tail_probe, dim3((m + 255) / 256), dim3(256), 0, 0, m, c, f, l, o);
        });
    });
}

// ---- the drop-off subdivisions (RR:4026-4062) ----
static double g_sd_ms[5] = {0, 0, 0, 0, 0};

extern "C" int pgr_last_subdivision_timing(double *ms5)
{
    if (!ms5) return PWR_ERR_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = g_sd_ms[i];
    return PWR_OK;
}

extern "C" void pgr_subdivision_free(pgr_subdivision *o)
{
    if (!o) return;
    free(o->dropoff_labels); free(o->reldrop_labels); free(o->winner); free(o->winner_cutoff);
    memset(o, 0, sizeof *o);
}

static int subdivide(const pgr_window *win, const pgr_result *r, int mincov, int device, pgr_subdivision *out)
{
    const int rows = win->rows, T = win->kept_rows, sc = win->sc, mingroup = mincov / 2;   // RR:4028
    const size_t V = (size_t)win->width * 5;
    out->rows = rows; out->kept_rows = T;
    out->dropoff_labels = (int *)malloc(sizeof(int) * (size_t)(rows ? rows : 1));
    out->reldrop_labels = (int *)malloc(sizeof(int) * (size_t)(rows ? rows : 1));
    if (!out->dropoff_labels || !out->reldrop_labels) return PWR_ERR_NOMEM;
    for (int i = 0; i < 5; ++i) g_sd_ms[i] = 0;
    // the selected entries, ascending (RR:3279-3286), and their cliques: -1 terminated within 31 entries, members inside the window
    std::vector<int> sel;
    for (int s = 0; s < r->nsig; ++s) {
        const int v = r->significant[s];
        if (v < 0 || (size_t)v >= V) return PWR_ERR_ARG;
        if (!(r->maxcorrs[v] > r->cutoff && r->sizes[s] > -1)) continue;
        const int *cl = r->cliques + (size_t)s * (PGR_MAXCLIQUE + 1);
        int nall = 0;
        while (nall <= PGR_MAXCLIQUE && cl[nall] >= 0) { if ((size_t)cl[nall] >= V) return PWR_ERR_ARG; nall++; }
        if (nall > PGR_MAXCLIQUE || r->sizes[s] > nall) return PWR_ERR_ARG;
        sel.push_back(s);
    }
    const int nsel = (int)sel.size();
    out->selected = nsel;
    std::vector<int> U((size_t)T + 1);
    double ms2[2] = {0, 0};
    int number = 0;
    int rc = pgr_dropoff_subdivision(r, mingroup, U.data(), &number, ms2);                   // RR:4037
    if (rc) return rc;
    g_sd_ms[0] = ms2[0]; g_sd_ms[1] = ms2[1];
    if ((rc = pgr_complete_labels(rows, win->kept, U.data(), out->dropoff_labels))) return rc;   // RR:4047
    number = pgr_compress_labels(T, U.data());                                               // RR:3288
    if (number < 0) return number;
    out->dropoff_parts = number;
    const size_t n1 = number ? number : 1;
    out->winner = (int *)malloc(sizeof(int) * n1); out->winner_cutoff = (int *)malloc(sizeof(int) * n1);
    if (!out->winner || !out->winner_cutoff) return PWR_ERR_NOMEM;
    for (size_t k = 0; k < n1; ++k) out->winner[k] = out->winner_cutoff[k] = -1;
    // the partitions that can split at all (RR:3300-3303), numbered 0 .. E - 1 for the device
    std::vector<int> count(n1, 0), eidx(n1, -1), part;
    for (int j = 0; j < T; ++j) count[U[j]]++;
    for (int k = 0; k < number; ++k)
        if (count[k] > mingroup * 2) { eidx[k] = (int)part.size(); part.push_back(k); }
    const int E = (int)part.size();
    out->eligible = E;
    std::vector<unsigned int> best((size_t)(E ? E : 1), 0xffffffffu);
    if (nsel > 0 && E > 0) {
        const double t0 = now_ms();
        if (T > 65535) return PWR_ERR_RANGE;                           // the kernel's 16-bit halves (pgr_read_window allows 30 000)
        if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
        // only the variations that are members of a selected clique go to the device, word-major as in pgr_refine
        std::vector<int> col(V, -1), used;
        std::vector<int> selcl((size_t)nsel * (PGR_MAXCLIQUE + 1), -1), selsz(nsel);
        for (int q = 0; q < nsel; ++q) {
            const int *cl = r->cliques + (size_t)sel[q] * (PGR_MAXCLIQUE + 1);
            for (int m = 0; m <= PGR_MAXCLIQUE && cl[m] >= 0; ++m) {
                if (col[cl[m]] < 0) { col[cl[m]] = (int)used.size(); used.push_back(cl[m]); }
                selcl[(size_t)q * (PGR_MAXCLIQUE + 1) + m] = col[cl[m]];
            }
            selsz[q] = r->sizes[sel[q]];
        }
        const size_t Vc = used.size();
        std::vector<unsigned long long> Gt((Vc ? Vc : 1) * sc);
        pgr_word_major(win->groups, sc, used.data(), Vc, Gt.data());
        std::vector<int> lab((size_t)sc * 64, -1);
        for (int j = 0; j < T; ++j) lab[j] = eidx[U[j]];
        DevArena dev;
        const unsigned long long *d_G = dev.put(Gt.data(), Gt.size());
        const int *d_selcl = dev.put(selcl.data(), selcl.size()), *d_selsz = dev.put(selsz.data(), nsel), *d_lab = dev.put(lab.data(), lab.size());
        unsigned int *d_best = dev.get<unsigned int>(E);
        if (!d_G || !d_selcl || !d_selsz || !d_lab || !d_best) return dev.err;
        HIPC(hipMemset(d_best, 0xff, (size_t)E * 4));
        HIPC(hipDeviceSynchronize());
        const double t1 = now_ms();
        hipLaunchKernelGGL(k_gr_reldrop, dim3(nsel), dim3(256), 0, 0, (int)Vc, sc, T, E, mingroup, d_selcl, d_selsz, d_lab, d_G, d_best);
        HIPC(hipGetLastError());
        HIPC(hipDeviceSynchronize());
        HIPC(hipMemcpy(best.data(), d_best, (size_t)E * 4, hipMemcpyDeviceToHost));
        g_sd_ms[2] = t1 - t0; g_sd_ms[3] = now_ms() - t1;
    }
    const double t2 = now_ms();
    // CliqueGroup(Clique, c) for the winners only (RR:3312), restricted to the rows of their partition, and the split (RR:3353-3362)
    for (int e = 0; e < E; ++e) {
        if (best[e] == 0xffffffffu) continue;
        const int q = (int)(best[e] >> 5), c = (int)(best[e] & 31u), k = part[e];
        if (q >= nsel) return PWR_ERR_INTERNAL;
        const int *cl = r->cliques + (size_t)sel[q] * (PGR_MAXCLIQUE + 1);
        for (int j = 0; j < T; ++j) {
            if (U[j] != k) continue;
            int ii = 0;
            for (int m = 0; m <= PGR_MAXCLIQUE && cl[m] >= 0; ++m) ii += (int)((win->groups[(size_t)cl[m] * sc + j / 64] >> (j % 64)) & 1ull);
            U[j] = ii > c ? number + 1 + k * 2 : number + 2 + k * 2;
        }
        out->winner[k] = r->significant[sel[q]];
        out->winner_cutoff[k] = c;
    }
    const int after = pgr_compress_labels(T, U.data());                                      // RR:3371
    if (after < 0) return after;
    out->reldrop_parts = after;
    if ((rc = pgr_complete_labels(rows, win->kept, U.data(), out->reldrop_labels))) return rc;   // RR:4061
    g_sd_ms[4] = now_ms() - t2;
    return PWR_OK;
}

extern "C" int pgr_subdivide(const pgr_window *win, const pgr_result *refined, int mincov, int device, pgr_subdivision *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!win || !refined || mincov < 0 || !win->kept || !win->groups) return PWR_ERR_ARG;
    if (win->rows != refined->rows || win->kept_rows != refined->kept_rows || win->sc != refined->sc || win->width != refined->width) return PWR_ERR_ARG;
    if (win->rows < 0 || win->kept_rows < 0 || win->kept_rows > win->rows || win->width <= 0 || win->sc != win->kept_rows / 64 + 1 || refined->nsig < 0) return PWR_ERR_ARG;
    if (refined->nsig > 0 && (!refined->significant || !refined->maxcorrs || !refined->sizes || !refined->cliques || !refined->drop_off || !refined->c_groups)) return PWR_ERR_ARG;
    const int rc = abi_guard([&] { return subdivide(win, refined, mincov, device, out); });
    if (rc) pgr_subdivision_free(out);
    return rc;
}
