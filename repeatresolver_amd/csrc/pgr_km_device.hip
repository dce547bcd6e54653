// pgr_km_device.hip -- MI355X (gfx950) implementation of RepeatResolver's last subdivision stage behind include/pgr.h.
//
// Reference: PhilippBongartz/RepeatResolver, RepeatResolver.c ("RR:"), Kmeans_Subdivision (RR:3382-3403): every part of the
// rows with more than 2 * mingroup members gets its variables (Relative_Vars, RR:2424-2493: the variations over the cutoff
// that at least mingroup rows of the part hold and that are significantly linked INSIDE the part with a variation at least
// 100 indices away) and is clustered on them (Kmeans, RR:2604-2821).  The parts do not see each other (a part hands out
// labels above every label present, and the loop's bound is fixed before it), so all of them go through each kernel at once.
//   k_km_counts     |G_c & U_e| for every (eligible part e, variation c over the cutoff): the mingroup filter, and gr1 / gr2.
//   k_km_pairs      the relative significance (RR:506-522, RR:490-504): a thread owns one variation a of a part and meets
//                   every partner b of the part, a tile of PKM_TB partners (AND-ed with the part's rows) staged in LDS per
//                   chunk of words; of a pair 100 or more apart it takes Z with the higher index as Groups[j], and keeps
//                   the maximum -- "any partner over the cutoff" is a max-reduction.  Every pair is met from both sides with
//                   the same arguments.  The partners are split over the grid's z (PKM_ZB per block) so that a part of a few
//                   thousand variations fills the device; the blocks of a variation join their maxima with an integer
//                   atomic max on the bits of the double (never negative), so the result does not depend on the order.
//   k_km_centroids  a thread per row i of a part walks j ascending, tiles of VarSigs staged in LDS, and keeps the five-slot
//                   list of RR:2658-2688 in registers: the exchange sort before every j, then slot 0 replaced -- swap for
//                   swap, since ties decide.  The centroid is the bitwise majority (3 of 5) of the five rows' words.
//   k_km_assign     first maximum over j != i of GrMatch(Centroids[j], VarSigs[i]) (RR:2706-2723); where the chain will
//                   run it also stores every score (16 bits) for the host, which walks RR:2726-2755 (pgr_kmeans_reassign).
// GrMatch (RR:163-175) under the temporary sc = varzahl / 64 + 1 (RR:2625) is sc * 64 - popcount(xor): the unused bits of the
// last word are 0 in both operands and count as matches.
// Compiled with -ffp-contract=off like pgr_device.hip: the tails are sums of products that must not fuse differently per site.
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
#include "hyper_tail.h"
#include "pgr.h"
#include "pgr_internal.h"

#define PKM_NT 256                  // threads per block
#define PKM_TB 16                   // partners per tile of k_km_pairs
#define PKM_ZB 64                   // partners per block of k_km_pairs (the grid's z runs over them)
#define PKM_WC 32                   // words per LDS chunk of k_km_pairs
#define PKM_LDS_WORDS 4096          // LDS tile of VarSigs / Centroids: 32 KB
#define PKM_MIN_DISTANCE 100        // RR:2462
#define PKM_MAX_SC 1023             // sc_km * 64 <= 65535: a score fits 16 bits
#define PKM_MAX_SCORES (1ull << 28) // entries of all score matrices together
#define PKM_MAX_DEBUG (1ull << 24)  // entries of the debug matrices / pairs returned
#define PKM_MAX_LABEL (1 << 24)     // labels accepted from the caller (Unterteilungskomprimierung allocates max + 1)

typedef unsigned long long u64;

static double g_km_ms[6] = {0, 0, 0, 0, 0, 0};

// grid (tiles of candidates, parts); G[w][c] over the nC candidates, U[e][w]
__global__ __launch_bounds__(PKM_NT) void k_km_counts(int nC, int sc, const u64 *__restrict__ G, const u64 *__restrict__ U, int *__restrict__ cnt)
{
    const int c = blockIdx.x * PKM_NT + threadIdx.x, e = blockIdx.y;
    if (c >= nC) return;
    int n = 0;
    for (int w = 0; w < sc; ++w) n += __popcll(G[(size_t)w * nC + c] & U[(size_t)e * sc + w]);
    cnt[(size_t)e * nC + c] = n;
}

// RR:506-522 with CumHypGeo_Log (RR:490-504) from the counts
// The counts k_km_pairs hands over stay inside what the table covers (hyper_probe_counts_ok states the inequalities): cov is
// the number of rows of the part U_e (at most the kept rows, the table's reach), gr1 and gr2 are |G & U_e| of the two
// variations (k_km_counts), subsets of U_e, and schnitt = |G_a & G_b & U_e| is the size of their intersection:
// schnitt <= min(gr1, gr2) and gr1 + gr2 - schnitt = |union| <= cov.  At schnitt == 0 the Q side gets k = 2^32 - 1, which
// d_hyper_Q answers with 0 before any lookup (k >= n1).
__device__ __noinline__ double d_km_significance(const double *__restrict__ lnf, int schnitt, int cov, int gr1, int gr2)
{
    if (gr1 == 0 || gr2 == 0) return 0.0;
    const double posP = d_hyper_P(lnf, (unsigned)schnitt, (unsigned)gr2, (unsigned)(cov - gr2), (unsigned)gr1);       // RR:492
    const double posQ = d_hyper_Q(lnf, (unsigned)schnitt - 1u, (unsigned)gr2, (unsigned)(cov - gr2), (unsigned)gr1);  // RR:493: wraps at 0
    double Z = -1.0 * log10((posP < posQ || schnitt == 0) ? posP : posQ);                                             // RR:495-503
    if (isinf(Z) || Z > 99) Z = 99.0;
    return Z;
}

// grid (tiles of a part's variations, parts, PKM_ZB partners each); maxZ is zeroed by the host.
// poff[e] .. poff[e + 1]: the part's variations (ascending): pcol = column in
// G, pvar = variation index, pgr = |G & U_e|.  dbg (may be null): per part a matrix [n][n] at doff[e], entry (a, b) for b the
// higher index.
__global__ __launch_bounds__(PKM_NT) void k_km_pairs(int nC, int sc, const int *__restrict__ poff, const int *__restrict__ pcol,
                                                     const int *__restrict__ pvar, const int *__restrict__ pgr, const int *__restrict__ pcov,
                                                     const u64 *__restrict__ G, const u64 *__restrict__ U, const double *__restrict__ lnf,
                                                     double *__restrict__ maxZ, const u64 *__restrict__ doff, double *__restrict__ dbg)
{
    __shared__ u64 sB[PKM_TB][PKM_WC];
    __shared__ int sVar[PKM_TB], sGr[PKM_TB], sCol[PKM_TB];
    const int e = blockIdx.y, tid = threadIdx.x, p0 = poff[e], n = poff[e + 1] - p0, a = blockIdx.x * PKM_NT + tid;
    const int bfrom = blockIdx.z * PKM_ZB, bto = min(n, bfrom + PKM_ZB);
    if (blockIdx.x * PKM_NT >= n || bfrom >= n) return;                // (the whole block)
    const bool have = a < n;
    const int mycol = have ? pcol[p0 + a] : 0, va = have ? pvar[p0 + a] : 0, ga = have ? pgr[p0 + a] : 0, cov = pcov[e];
    double best = 0.0;
    for (int b0 = bfrom; b0 < bto; b0 += PKM_TB) {
        int s[PKM_TB];
#pragma unroll
        for (int t = 0; t < PKM_TB; ++t) s[t] = 0;
        __syncthreads();                                               // (everyone is done with the tile before)
        if (tid < PKM_TB) {
            const bool ok = b0 + tid < n;
            sVar[tid] = ok ? pvar[p0 + b0 + tid] : 0; sGr[tid] = ok ? pgr[p0 + b0 + tid] : 0; sCol[tid] = ok ? pcol[p0 + b0 + tid] : -1;
        }
        for (int w0 = 0; w0 < sc; w0 += PKM_WC) {
            __syncthreads();
            for (int t = tid; t < PKM_TB * PKM_WC; t += PKM_NT) {
                const int tb = t / PKM_WC, w = w0 + t % PKM_WC, col = sCol[tb];
                sB[tb][t % PKM_WC] = (col >= 0 && w < sc) ? (G[(size_t)w * nC + col] & U[(size_t)e * sc + w]) : 0ull;
            }
            __syncthreads();
            if (have) {
                const int wn = min(PKM_WC, sc - w0);
                for (int w = 0; w < wn; ++w) {
                    const u64 g = G[(size_t)(w0 + w) * nC + mycol];
#pragma unroll
                    for (int t = 0; t < PKM_TB; ++t) s[t] += __popcll(g & sB[t][w]);
                }
            }
        }
        if (have) {
#pragma unroll
            for (int t = 0; t < PKM_TB; ++t) {
                const int b = b0 + t;
                if (b >= n) continue;
                const int vb = sVar[t], gb = sGr[t];
                if (vb >= va + PKM_MIN_DISTANCE) {                     // i = a, j = b: (Groups[j], Groups[i], U)
                    const double Z = d_km_significance(lnf, s[t], cov, gb, ga);
                    if (Z > best) best = Z;
                    if (dbg) dbg[doff[e] + (size_t)a * n + b] = Z;
                } else if (va >= vb + PKM_MIN_DISTANCE) {              // i = b, j = a
                    const double Z = d_km_significance(lnf, s[t], cov, ga, gb);
                    if (Z > best) best = Z;
                }
            }
        }
    }
    // best is +0.0 or a positive finite number: its bits order as the values do
    if (have && best > 0.0) atomicMax(reinterpret_cast<u64 *>(maxZ + p0 + a), (u64)__double_as_longlong(best));
}

// what every part of the k-means kernels needs: its rows, its words and where its arrays start
struct KmPart {
    int anzahl, sc_km;
    u64 voff;                       // into VarSigs / Centroids: [w][i], anzahl entries per word
    u64 soff;                       // into the score matrices: [i][j]
    int roff;                       // into the per-row outputs
};

__device__ __forceinline__ u64 maj3of5(u64 a, u64 b, u64 c, u64 d, u64 e)
{
    return (a & b & c) | (a & b & d) | (a & b & e) | (a & c & d) | (a & c & e) | (a & d & e) | (b & c & d) | (b & c & e) | (b & d & e) | (c & d & e);
}

// stages the rows j0 .. j0 + tj of X (word-major, per part) as sV[jl * sc_km + w]; consecutive threads read consecutive rows
__device__ __forceinline__ void km_stage(u64 *sV, const u64 *__restrict__ X, const KmPart &p, int j0, int tj, int tid)
{
    for (int t = tid; t < tj * p.sc_km; t += PKM_NT) {
        const int w = t / tj, jl = t - w * tj;
        sV[jl * p.sc_km + w] = j0 + jl < p.anzahl ? X[p.voff + (size_t)w * p.anzahl + j0 + jl] : 0ull;
    }
}

// GrMatch(row jl of the tile, VarSigs[i]); v0 = word 0 of VarSigs[i]
__device__ __forceinline__ int km_match(const u64 *sV, const u64 *__restrict__ VS, const KmPart &p, int jl, int i, u64 v0)
{
    int d = __popcll(sV[jl * p.sc_km] ^ v0);
    for (int w = 1; w < p.sc_km; ++w) d += __popcll(sV[jl * p.sc_km + w] ^ VS[p.voff + (size_t)w * p.anzahl + i]);
    return p.sc_km * 64 - d;
}

// grid (tiles of a part's rows, parts)
__global__ __launch_bounds__(PKM_NT) void k_km_centroids(const KmPart *__restrict__ parts, const u64 *__restrict__ VS, u64 *__restrict__ CT)
{
    __shared__ u64 sV[PKM_LDS_WORDS];
    const KmPart p = parts[blockIdx.y];
    const int tid = threadIdx.x, i = blockIdx.x * PKM_NT + tid;
    if (blockIdx.x * PKM_NT >= p.anzahl) return;                       // (the whole block)
    const bool have = i < p.anzahl;
    const int tj = PKM_LDS_WORDS / p.sc_km;                            // >= 4: sc_km <= PKM_MAX_SC (checked by the host)
    const u64 v0 = have ? VS[p.voff + i] : 0ull;
    int bs0 = 0, bs1 = 0, bs2 = 0, bs3 = 0, bs4 = 0, bj0 = 0, bj1 = 0, bj2 = 0, bj3 = 0, bj4 = 0;   // RR:2658-2662
#define PKM_SWAP(l, k)                                                                             \
    if (bs##l < bs##k) { int s_ = bs##l; bs##l = bs##k; bs##k = s_; s_ = bj##l; bj##l = bj##k; bj##k = s_; }
    for (int j0 = 0; j0 < p.anzahl; j0 += tj) {
        __syncthreads();
        km_stage(sV, VS, p, j0, tj, tid);
        __syncthreads();
        if (have) {
            const int jn = min(tj, p.anzahl - j0);
            for (int jl = 0; jl < jn; ++jl) {
                const int score = km_match(sV, VS, p, jl, i, v0);      // RR:2666
                PKM_SWAP(1, 0) PKM_SWAP(2, 0) PKM_SWAP(3, 0) PKM_SWAP(4, 0)        // RR:2667-2681: k = 0, l = 1 .. 4
                PKM_SWAP(2, 1) PKM_SWAP(3, 1) PKM_SWAP(4, 1)                       // k = 1
                PKM_SWAP(3, 2) PKM_SWAP(4, 2)                                      // k = 2
                PKM_SWAP(4, 3)                                                     // k = 3
                if (score > bs0) { bs0 = score; bj0 = j0 + jl; }       // RR:2682-2687
            }
        }
    }
#undef PKM_SWAP
    if (have)
        for (int w = 0; w < p.sc_km; ++w) {                            // RR:2694-2702: in more than 2 of the five rows
            const u64 *x = VS + p.voff + (size_t)w * p.anzahl;
            CT[p.voff + (size_t)w * p.anzahl + i] = maj3of5(x[bj0], x[bj1], x[bj2], x[bj3], x[bj4]);
        }
}

// grid (tiles of a part's rows, parts); S (may be null): the scores for the chain
__global__ __launch_bounds__(PKM_NT) void k_km_assign(const KmPart *__restrict__ parts, const u64 *__restrict__ VS, const u64 *__restrict__ CT,
                                                      int *__restrict__ cluster, unsigned short *__restrict__ S)
{
    __shared__ u64 sV[PKM_LDS_WORDS];
    const KmPart p = parts[blockIdx.y];
    const int tid = threadIdx.x, i = blockIdx.x * PKM_NT + tid;
    if (blockIdx.x * PKM_NT >= p.anzahl) return;                       // (the whole block)
    const bool have = i < p.anzahl;
    const int tj = PKM_LDS_WORDS / p.sc_km;
    const u64 v0 = have ? VS[p.voff + i] : 0ull;
    int best_score = 0, best_j = 0;                                    // RR:2708-2709
    for (int j0 = 0; j0 < p.anzahl; j0 += tj) {
        __syncthreads();
        km_stage(sV, CT, p, j0, tj, tid);
        __syncthreads();
        if (have) {
            const int jn = min(tj, p.anzahl - j0);
            for (int jl = 0; jl < jn; ++jl) {
                const int j = j0 + jl, score = km_match(sV, VS, p, jl, i, v0);     // RR:2712
                if (score > best_score && i != j) { best_score = score; best_j = j; }
                if (S) S[p.soff + (size_t)i * p.anzahl + j] = (unsigned short)score;
            }
        }
    }
    if (have) cluster[p.roff + i] = best_j;                            // RR:2721
}

namespace {
template <class T> T *km_copy(const std::vector<T> &v)
{
    T *p = (T *)malloc(sizeof(T) * (v.size() ? v.size() : 1));
    if (p && !v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}
}   // namespace

extern "C" int pgr_last_kmeans_timing(double *ms6)
{
    if (!ms6) return PWR_ERR_ARG;
    for (int i = 0; i < 6; ++i) ms6[i] = g_km_ms[i];
    return PWR_OK;
}

extern "C" void pgr_kmeans_free(pgr_kmeans *o)
{
    if (!o) return;
    free(o->labels); free(o->part); free(o->part_rows); free(o->row_offset); free(o->row); free(o->cluster_before); free(o->cluster_after);
    free(o->varzahl); free(o->var_offset); free(o->vars); free(o->pair_part); free(o->pair_i); free(o->pair_j); free(o->pair_z);
    memset(o, 0, sizeof *o);
}

static int kmeans(const pgr_window *win, const pgr_result *r, const int *labels_rows, int mincov, int device, bool want_pairs, pgr_kmeans *out)
{
    const double t0 = now_ms();
    const int rows = win->rows, T = win->kept_rows, sc = win->sc, mingroup = mincov / 2;       // RR:4028
    const size_t V = (size_t)win->width * 5;
    for (int i = 0; i < 6; ++i) g_km_ms[i] = 0;
    out->rows = rows; out->kept_rows = T;
    std::vector<int> U;
    U.reserve((size_t)T + 1);
    for (int i = 0; i < rows; ++i) {
        if (labels_rows[i] < -1) return PWR_ERR_ARG;
        if (!win->kept[i]) continue;
        if (labels_rows[i] < 0 || labels_rows[i] > PKM_MAX_LABEL || (int)U.size() >= T) return PWR_ERR_ARG;
        U.push_back(labels_rows[i]);
    }
    if ((int)U.size() != T) return PWR_ERR_ARG;
    U.push_back(0);                                                    // (data() of an empty vector)
    int number = pgr_compress_labels(T, U.data());                     // RR:3385
    if (number < 0) return number;
    out->parts_before = number;
    std::vector<int> count((size_t)number + 1, 0), part;
    for (int j = 0; j < T; ++j) count[U[j]]++;
    for (int k = 0; k < number; ++k)
        if (count[k] > mingroup * 2) part.push_back(k);                // RR:3391
    const int E = (int)part.size();
    if (E > 65535) return PWR_ERR_RANGE;                               // the parts are the grids' y dimension
    out->eligible = E;
    // the rows of every eligible part, ascending (RR:2616-2623)
    std::vector<int> eidx((size_t)number + 1, -1), roff((size_t)E + 1, 0), prow;
    for (int e = 0; e < E; ++e) { eidx[part[e]] = e; roff[e + 1] = roff[e] + count[part[e]]; }
    prow.resize((size_t)roff[E]);
    {
        std::vector<int> fill(roff.begin(), roff.end() - 1);
        for (int j = 0; j < T; ++j)
            if (eidx[U[j]] >= 0) prow[fill[eidx[U[j]]]++] = j;
    }
    std::vector<int> voff((size_t)E + 1, 0), vars, before((size_t)roff[E], 0), after((size_t)roff[E], 0), dpart, dpi, dpj;
    std::vector<double> dpz;
    long long npairs = 0;
    if (E > 0) {
        if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
        DevArena d;
        // ---- Relative_Vars: the variations over the cutoff (RR:2430-2434), word-major as in pgr_refine ----
        std::vector<int> cand;
        for (size_t v = 0; v < V; ++v)
            if (r->maxcorrs[v] > r->cutoff) cand.push_back((int)v);
        const int nC = (int)cand.size();
        std::vector<u64> Gc((size_t)(nC ? nC : 1) * sc), Ue((size_t)E * sc, 0ull);
        pgr_word_major(win->groups, sc, cand.data(), (size_t)nC, Gc.data());
        for (int e = 0; e < E; ++e)
            for (int q = roff[e]; q < roff[e + 1]; ++q) Ue[(size_t)e * sc + prow[q] / 64] |= 1ull << (prow[q] % 64);   // RR:2438
        std::vector<int> poff((size_t)E + 1, 0), pcol, pvar, pgr_, pcov(E);
        std::vector<double> maxZ;
        if (nC > 0) {
            const u64 *dG = d.put(Gc.data(), Gc.size()), *dU = d.put(Ue.data(), Ue.size());
            int *dcnt = d.get<int>((size_t)E * nC);
            if (!dG || !dU || !dcnt) return d.err;
            hipLaunchKernelGGL(k_km_counts, dim3((nC + PKM_NT - 1) / PKM_NT, E), dim3(PKM_NT), 0, 0, nC, sc, dG, dU, dcnt);
            HIPC(hipGetLastError());
            std::vector<int> cnt((size_t)E * nC);
            HIPC(hipMemcpy(cnt.data(), dcnt, cnt.size() * 4, hipMemcpyDeviceToHost));
            int nmax = 0;
            u64 dtotal = 0;
            std::vector<u64> doff(E);
            for (int e = 0; e < E; ++e) {
                pcov[e] = count[part[e]];
                for (int c = 0; c < nC; ++c)
                    if (cnt[(size_t)e * nC + c] >= mingroup) { pcol.push_back(c); pvar.push_back(cand[c]); pgr_.push_back(cnt[(size_t)e * nC + c]); }   // RR:2448
                poff[e + 1] = (int)pcol.size();
                const int n = poff[e + 1] - poff[e];
                nmax = std::max(nmax, n);
                doff[e] = dtotal; dtotal += (u64)n * n;
                for (int a = poff[e], b = poff[e]; a < poff[e + 1]; ++a) {           // pairs (i, j >= i + 100)
                    while (b < poff[e + 1] && pvar[b] < pvar[a] + PKM_MIN_DISTANCE) ++b;
                    npairs += poff[e + 1] - b;
                }
            }
            if ((nmax + PKM_ZB - 1) / PKM_ZB > 65535) return PWR_ERR_RANGE;          // the partners are the grid's z dimension
            if (want_pairs && (dtotal > PKM_MAX_DEBUG || (u64)npairs > PKM_MAX_DEBUG)) return PWR_ERR_RANGE;
            g_km_ms[1] = now_ms() - t0;
            const double t1 = now_ms();
            const size_t np = pcol.size();
            maxZ.assign(np, 0.0);
            if (nmax > 0) {
                const std::vector<double> lnf = hyper_lnf_table(T);
                const int *dpoff = d.put(poff.data(), poff.size()), *dpcol = d.put(pcol.data(), np), *dpvar = d.put(pvar.data(), np),
                          *dpgr = d.put(pgr_.data(), np), *dpcov = d.put(pcov.data(), E);
                const double *dlnf = d.put(lnf.data(), lnf.size());
                const u64 *ddoff = d.put(doff.data(), E);
                double *dmaxZ = d.get<double>(np), *ddbg = nullptr;
                if (!dpoff || !dpcol || !dpvar || !dpgr || !dpcov || !dlnf || !dmaxZ || !ddoff) return d.err;
                if (want_pairs) {
                    if (!(ddbg = d.get<double>((size_t)dtotal))) return PWR_ERR_NOMEM;
                    HIPC(hipMemset(ddbg, 0, (size_t)(dtotal ? dtotal : 1) * 8));
                }
                HIPC(hipMemset(dmaxZ, 0, (np ? np : 1) * 8));
                HIPC(hipDeviceSynchronize());
                const double t1b = now_ms();
                g_km_ms[1] += t1b - t1;
                hipLaunchKernelGGL(k_km_pairs, dim3((nmax + PKM_NT - 1) / PKM_NT, E, (nmax + PKM_ZB - 1) / PKM_ZB), dim3(PKM_NT), 0, 0, nC, sc, dpoff, dpcol, dpvar, dpgr, dpcov, dG, dU,
                                   dlnf, dmaxZ, ddoff, ddbg);
                HIPC(hipGetLastError());
                HIPC(hipDeviceSynchronize());
                g_km_ms[2] = now_ms() - t1b;
                HIPC(hipMemcpy(maxZ.data(), dmaxZ, np * 8, hipMemcpyDeviceToHost));
                if (want_pairs && dtotal > 0) {
                    std::vector<double> dbg((size_t)dtotal);
                    HIPC(hipMemcpy(dbg.data(), ddbg, (size_t)dtotal * 8, hipMemcpyDeviceToHost));
                    for (int e = 0; e < E; ++e) {
                        const int n = poff[e + 1] - poff[e];
                        for (int a = 0; a < n; ++a)
                            for (int b = a + 1; b < n; ++b)
                                if (pvar[poff[e] + b] >= pvar[poff[e] + a] + PKM_MIN_DISTANCE) {
                                    dpart.push_back(e); dpi.push_back(pvar[poff[e] + a]); dpj.push_back(pvar[poff[e] + b]);
                                    dpz.push_back(dbg[doff[e] + (size_t)a * n + b]);
                                }
                    }
                }
            }
        }
        // the marked variations (RR:2468-2472, RR:2486): a variation is marked iff one of its pairs is over the cutoff
        for (int e = 0; e < E; ++e) {
            for (int a = poff[e]; a < poff[e + 1]; ++a)
                if (maxZ[a] > r->cutoff) vars.push_back(pvar[a]);
            voff[e + 1] = (int)vars.size();
        }
        // ---- Kmeans: VarSigs (RR:2633-2640), word-major per part ----
        const double t2 = now_ms();
        const bool chain = mingroup > 2;                               // RR:2727: min = 2 .. mingroup - 1
        std::vector<KmPart> kp(E);
        u64 words = 0, scores = 0;
        int amax = 0;
        for (int e = 0; e < E; ++e) {
            const int anzahl = roff[e + 1] - roff[e], varzahl = voff[e + 1] - voff[e], sc_km = varzahl / 64 + 1;     // RR:2625
            if (sc_km > PKM_MAX_SC) return PWR_ERR_RANGE;
            kp[e] = KmPart{anzahl, sc_km, words, scores, roff[e]};
            words += (u64)anzahl * sc_km;
            if (chain) scores += (u64)anzahl * anzahl;
            amax = std::max(amax, anzahl);
        }
        if (scores > PKM_MAX_SCORES) return PWR_ERR_RANGE;
        std::vector<u64> VS((size_t)words, 0ull);
        for (int e = 0; e < E; ++e)
            for (int j = voff[e]; j < voff[e + 1]; ++j) {
                const u64 *g = win->groups + (size_t)vars[j] * sc;
                const int jj = j - voff[e];
                u64 *dst = VS.data() + kp[e].voff + (size_t)(jj / 64) * kp[e].anzahl;
                for (int i = 0; i < kp[e].anzahl; ++i) {
                    const int row = prow[roff[e] + i];
                    dst[i] |= ((g[row / 64] >> (row % 64)) & 1ull) << (jj % 64);
                }
            }
        const KmPart *dkp = d.put(kp.data(), E);
        const u64 *dVS = d.put(VS.data(), (size_t)words);
        u64 *dCT = d.get<u64>((size_t)words);
        int *dcl = d.get<int>((size_t)roff[E]);
        unsigned short *dS = chain ? d.get<unsigned short>((size_t)scores) : nullptr;
        if (!dkp || !dVS || !dCT || !dcl || (chain && !dS)) return d.err;
        const dim3 grid((amax + PKM_NT - 1) / PKM_NT, E);
        hipLaunchKernelGGL(k_km_centroids, grid, dim3(PKM_NT), 0, 0, dkp, dVS, dCT);
        HIPC(hipGetLastError());
        hipLaunchKernelGGL(k_km_assign, grid, dim3(PKM_NT), 0, 0, dkp, dVS, dCT, dcl, dS);
        HIPC(hipGetLastError());
        HIPC(hipMemcpy(before.data(), dcl, before.size() * 4, hipMemcpyDeviceToHost));
        std::vector<unsigned short> S;
        if (chain) {
            S.resize((size_t)scores);
            HIPC(hipMemcpy(S.data(), dS, (size_t)scores * 2, hipMemcpyDeviceToHost));
        }
        const double t3 = now_ms();
        g_km_ms[3] = t3 - t2;
        after = before;
        int max_u = number > 0 ? number - 1 : 0;                       // RR:2813-2814
        for (int e = 0; e < E; ++e) {
            const int anzahl = kp[e].anzahl;
            int *cl = after.data() + roff[e];
            for (int i = 0; i < anzahl; ++i)
                if (cl[i] < 0 || cl[i] >= anzahl) return PWR_ERR_INTERNAL;
            if (chain) {
                const int rc = pgr_kmeans_reassign(anzahl, S.data() + kp[e].soff, mingroup, cl);
                if (rc) return rc;
            }
            const int base = max_u + 1;
            for (int i = 0; i < anzahl; ++i) {                         // RR:2815
                U[prow[roff[e] + i]] = base + cl[i];
                max_u = std::max(max_u, base + cl[i]);
            }
        }
        g_km_ms[4] = now_ms() - t3;
    }
    const int parts = pgr_compress_labels(T, U.data());                // RR:3398
    if (parts < 0) return parts;
    out->parts = parts;
    out->labels = (int *)malloc(sizeof(int) * (size_t)(rows ? rows : 1));
    if (!out->labels) return PWR_ERR_NOMEM;
    const int rc = pgr_complete_labels(rows, win->kept, U.data(), out->labels);              // RR:4074
    if (rc) return rc;
    std::vector<int> prows(E), vz(E);
    for (int e = 0; e < E; ++e) { prows[e] = roff[e + 1] - roff[e]; vz[e] = voff[e + 1] - voff[e]; }
    out->part = km_copy(part); out->part_rows = km_copy(prows); out->row_offset = km_copy(roff); out->row = km_copy(prow);
    out->cluster_before = km_copy(before); out->cluster_after = km_copy(after); out->varzahl = km_copy(vz); out->var_offset = km_copy(voff);
    out->vars = km_copy(vars); out->pair_part = km_copy(dpart); out->pair_i = km_copy(dpi); out->pair_j = km_copy(dpj); out->pair_z = km_copy(dpz);
    if (!out->part || !out->part_rows || !out->row_offset || !out->row || !out->cluster_before || !out->cluster_after || !out->varzahl ||
        !out->var_offset || !out->vars || !out->pair_part || !out->pair_i || !out->pair_j || !out->pair_z) return PWR_ERR_NOMEM;
    out->pairs = npairs;
    out->debug_pairs = (long long)dpz.size();
    g_km_ms[0] = now_ms() - t0; g_km_ms[5] = (double)npairs;
    return PWR_OK;
}

static int kmeans_checked(const pgr_window *win, const pgr_result *refined, const int *labels_rows, int mincov, int device, bool want_pairs,
                          pgr_kmeans *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!win || !refined || !labels_rows || mincov < 0 || !win->kept || !win->groups || !refined->maxcorrs) return PWR_ERR_ARG;
    if (win->rows != refined->rows || win->kept_rows != refined->kept_rows || win->sc != refined->sc || win->width != refined->width) return PWR_ERR_ARG;
    if (win->rows < 0 || win->kept_rows < 0 || win->kept_rows > win->rows || win->width <= 0 || win->sc != win->kept_rows / 64 + 1) return PWR_ERR_ARG;
    const int rc = abi_guard([&] { return kmeans(win, refined, labels_rows, mincov, device, want_pairs, out); });
    if (rc) pgr_kmeans_free(out);
    return rc;
}

// ---- test hook: the tail functions k_km_pairs calls, as this file compiles them, on given counts (thread = one tuple) ----
__global__ __launch_bounds__(256) void k_km_tail_probe(int n, const int *__restrict__ counts, const double *__restrict__ lnf, double *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int *c = counts + (size_t)t * 6;
    const int s = c[0], cov = c[1], g1 = c[2], g2 = c[3];
    double *o = out + (size_t)t * 3;
    o[0] = d_hyper_P(lnf, (unsigned)s, (unsigned)g2, (unsigned)(cov - g2), (unsigned)g1);
    o[1] = d_hyper_Q(lnf, (unsigned)s - 1u, (unsigned)g2, (unsigned)(cov - g2), (unsigned)g1);
    o[2] = d_km_significance(lnf, s, cov, g1, g2);
}

extern "C" int pgr_km_tail_probe(int n, const int *counts, const double *floor, int device, double *out)
{
    return abi_guard([&] {
        return hyper_probe_run(n, counts, floor, device, PGR_MAX_ROWS, 3, out, [](int m, const int *c, const double *, const double *l, double *o) {
            hipLaunchKernelGGL(k_km_tail_probe, dim3((m + 255) / 256), dim3(256), 0, 0, m, c, l, o);
        });
    });
}

extern "C" int pgr_kmeans_subdivide(const pgr_window *win, const pgr_result *refined, const int *reldrop_labels_rows, int mincov, int device,
                                    pgr_kmeans *out)
{
    return kmeans_checked(win, refined, reldrop_labels_rows, mincov, device, false, out);
}

extern "C" int pgr_kmeans_subdivide_pairs(const pgr_window *win, const pgr_result *refined, const int *reldrop_labels_rows, int mincov, int device,
                                          pgr_kmeans *out)
{
    return kmeans_checked(win, refined, reldrop_labels_rows, mincov, device, true, out);
}
