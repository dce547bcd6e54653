// four_count_tile.h -- the tiled bit-set product of k_mc_pairs (pmc_device.hip) and k_gr_cliques (pgr_device.hip): a tile of TA
// variations stays in LDS, WC words at a time (their group set and their column's coverage set); every thread owns one
// partner variation, streams its two sets once and keeps four intersection sizes per (tile member, partner) in registers.
// The sets are word-major: G[w][v] over V = 5 W variations, LC[w][column] over W columns, column = v / 5.
#ifndef PWR_FOUR_COUNT_TILE_H
#define PWR_FOUR_COUNT_TILE_H

#include <hip/hip_runtime.h>

// The words [w0, min(w0 + WC, wend)) of the tile's members s_v[TA] (-1: no such member) into sG / sL, zeros beyond; by all
// NT threads of the block, between two barriers of the caller's.
template <int TA, int WC, int NT>
__device__ __forceinline__ void tile_stage(unsigned long long (*sG)[WC], unsigned long long (*sL)[WC], const int *s_v,
                                           const unsigned long long *__restrict__ G, const unsigned long long *__restrict__ LC,
                                           int V, int W, int w0, int wend, int tid)
{
    for (int t = tid; t < TA * WC; t += NT) {
        const int a = t / WC, w = w0 + t % WC, v = s_v[a];
        const bool ok = v >= 0 && w < wend;
        sG[a][t % WC] = ok ? G[(size_t)w * V + v] : 0ull;
        sL[a][t % WC] = ok ? LC[(size_t)w * W + v / 5] : 0ull;
    }
}

// The staged words against partner p, for every member a of the tile: both[a] += |G_a & G_p|, in_p[a] += |G_a & LC_p|,
// in_a[a] += |G_p & LC_a|, cov[a] += |LC_a & LC_p|.
template <int TA, int WC>
__device__ __forceinline__ void tile_count(const unsigned long long (*sG)[WC], const unsigned long long (*sL)[WC],
                                           const unsigned long long *__restrict__ G, const unsigned long long *__restrict__ LC,
                                           int V, int W, int w0, int wend, int p, int *both, int *in_p, int *in_a, int *cov)
{
    const int wn = min(WC, wend - w0);
    size_t og = (size_t)w0 * V + p, ol = (size_t)w0 * W + p / 5;                     // the partner's sets, word w0 + w
    for (int w = 0; w < wn; ++w, og += V, ol += W) {
        const unsigned long long gp = G[og], lp = LC[ol];
#pragma unroll
        for (int a = 0; a < TA; ++a) {
            const unsigned long long ga = sG[a][w], la = sL[a][w];
            both[a] += __popcll(ga & gp); in_p[a] += __popcll(ga & lp); in_a[a] += __popcll(gp & la); cov[a] += __popcll(la & lp);
        }
    }
}

#endif /* PWR_FOUR_COUNT_TILE_H */
