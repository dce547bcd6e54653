// pfl_device.hip -- MI355X (gfx950) implementation of the flank distances behind include/pfl.h (pfl_distances) and, further
// down, of the placements with traceback and the votes (pfl_place, pfl_consensus).
//
// The distance of two flanks is an edit distance with unit costs whose start is anchored in both sequences, D(0,y) = y and
// D(x,0) = x, and whose end is free in the text: min over y of D(m,y) (pfl.h).  Neighbouring cells differ by -1, 0 or +1, so a
// column of the table is two bit vectors over the pattern (Pv: D(x,y) - D(x-1,y) = +1, Mv: = -1), advanced one text base per
// handful of integer instructions per 32 pattern rows: Myers 1999 in Hyyro's block form, the step of prc_device.hip and
// pia_device.hip, with three differences.  The horizontal delta carried into row 0 is +1 (D(0,y) - D(0,y-1) = 1), not 0; pattern
// and text both change from pair to pair; and of the last row only its minimum leaves the kernel.
//
// Layout: the flanks that are long enough are sorted by (a, index), and the pattern of a pair is the one that comes first, so
// in the triangle of pairs every row has ONE pattern.  A wave takes a tile = one pattern and 64 consecutive texts, a text per
// lane.  The pattern is then wave-uniform: its two bit planes are made by the wave itself from the pattern's bases (64 rows per
// ballot) and live in scalar registers, ceil(m / 32) words each, the kernel being compiled per word count; a lane keeps only
// Pv and Mv, 2 x 16 registers at most, and fetches its own text bases, eight at a time.  m is uniform too, so the word and the bit
// of row m - 1 whose delta moves the score are the same in every lane and the word is the last one of the instance: no
// register is indexed at run time.  Texts of one tile have between m and m + m / 4 bases: the lanes run the same steps but for
// a short tail.  No LDS, no barrier, no atomics; a lane owns its pair and the wave stores its 64 results side by side.
//
// Only the bases a distance can reach are on the device: per flank the min(len, reach + reach / 4) bytes nearest to the
// boundary, in the piece's own orientation, packed into one upload.  A flank carries its mode; the kernel walks backwards
// and flips bit 1 of the code (a c g t -> 0 1 3 2) where the mode says so, as k_rc_rows<.., BOTH> does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#define PWR_STAGE "pfl"
#include "dev_util.h"
#include "pfl.h"

#define FL_MAXW (PFL_MAX_REACH / 32)
#define FL_AHEAD 8                  // text bases fetched per wait
#define FL_SCRATCH_DEFAULT (1LL << 30)   // bytes of traceback scratch a context takes at most unless told otherwise
static_assert(FL_MAXW * 32 == PFL_MAX_REACH, "PFL_MAX_REACH is what the widest kernel holds");

struct FlFlank {                    // one flank of min_len or more, in sorted order
    int woff;                       // offset of its window in the packed bases
    int need;                       // bytes of the window: min(len, reach + reach / 4)
    int a;                          // min(len, reach)
    int mode;                       // bit 0: the anchored sequence runs from the window's last byte down; bit 1: complemented
};

// base y of a flank's anchored sequence, as the code a c g t -> 0 1 3 2
__device__ __forceinline__ int fl_code(const unsigned char *__restrict__ win, const FlFlank &f, int y)
{
    const int ch = win[f.woff + ((f.mode & 1) ? f.need - 1 - y : y)];
    return ((ch >> 1) & 3) ^ (f.mode & 2);
}

// one wave per tile {pattern (sorted position), first text (sorted position)}; lane l has text first + l
template <int NW>
__global__ __launch_bounds__(64) void k_fl_tiles(const unsigned char *__restrict__ win, const FlFlank *__restrict__ fl,
                                                 const int2 *__restrict__ tiles, int ns, int *__restrict__ dist)
{
    const int lane = threadIdx.x;
    const int2 tile = tiles[blockIdx.x];
    const FlFlank p = fl[tile.x];
    const int m = p.a;                                      // 32 * (NW - 1) < m <= 32 * NW
    // the pattern's planes: bit x of plane 0/1 = bit 0/1 of the code of pattern row x (rows past m - 1 hold an 'a': what a row
    // above m - 1 does never reaches the rows below it)
    uint32_t P0[NW], P1[NW];
#pragma unroll
    for (int h = 0; h < (NW + 1) / 2; ++h) {
        const int x = h * 64 + lane;
        const int code = x < m ? fl_code(win, p, x) : 0;
        const unsigned long long b0 = __ballot(code & 1), b1 = __ballot(code & 2);
        P0[2 * h] = (uint32_t)b0; P1[2 * h] = (uint32_t)b1;
        if (2 * h + 1 < NW) { P0[2 * h + 1] = (uint32_t)(b0 >> 32); P1[2 * h + 1] = (uint32_t)(b1 >> 32); }
    }
    const int js = tile.y + lane;
    const bool have = js < ns;
    const FlFlank t = fl[have ? js : tile.y];               // (a lane without a text walks the tile's first one and stores nothing)
    const int tl = min(t.need, m + (m >> 2));               // |T| = min(len_j, m + m / 4) >= m >= 1
    int steps = tl;
    for (int o = 32; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o));
    steps = __builtin_amdgcn_readfirstlane(steps);          // (the same in every lane: the loop is the wave's, not the lanes')
    const int bt = (m - 1) & 31;                            // row m - 1 is bit bt of word NW - 1
    uint32_t Pv[NW], Mv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) { Pv[w] = ~0u; Mv[w] = 0u; }   // column 0: D(x,0) - D(x-1,0) = +1
    int score = m, best = m;                                // D(m,0) = m
    // FL_AHEAD text bases per fetch: the loads of a run go out together and are waited for once.  Past |T| a lane fetches its
    // last base again and steps on; what it computes there is never looked at.
    for (int y0 = 0; y0 < steps; y0 += FL_AHEAD) {
        int cs[FL_AHEAD];
#pragma unroll
        for (int k = 0; k < FL_AHEAD; ++k) cs[k] = fl_code(win, t, min(y0 + k, tl - 1));
#pragma unroll
        for (int k = 0; k < FL_AHEAD; ++k) {
            const int cur = cs[k];
            const uint32_t r0 = (cur & 1) ? ~0u : 0u, r1 = (cur & 2) ? ~0u : 0u;
            uint32_t hp = 1u, hn = 0u, tp = 0u, tn = 0u;    // D(0,y+1) - D(0,y) = +1: the start is anchored in the text too
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t Eq = ~(P0[w] ^ r0) & ~(P1[w] ^ r1);
                const uint32_t Xv = Eq | Mv[w], Eqh = Eq | hn;
                const uint32_t Xh = (((Eqh & Pv[w]) + Pv[w]) ^ Pv[w]) | Eqh;
                uint32_t Ph = Mv[w] | ~(Xh | Pv[w]), Mh = Pv[w] & Xh;
                if (w == NW - 1) { tp = Ph; tn = Mh; }
                const uint32_t hp2 = Ph >> 31, hn2 = Mh >> 31;
                Ph = (Ph << 1) | hp; Mh = (Mh << 1) | hn;
                Pv[w] = Mh | ~(Xv | Ph);
                Mv[w] = Ph & Xv;
                hp = hp2; hn = hn2;
            }
            score += (int)((tp >> bt) & 1u) - (int)((tn >> bt) & 1u);   // D(m, y0 + k + 1)
            if (y0 + k < tl) best = min(best, score);
        }
    }
    if (have) dist[(size_t)tile.x * ns + js] = best;        // the upper triangle in sorted positions, 64 neighbours per wave
}

// ---------------------------------------------------------------------------------------------
// placement with traceback (pfl_place) and the votes of a cluster (pfl_consensus)
// ---------------------------------------------------------------------------------------------
// One word (32 pattern rows) of one column: k_fl_tiles's step, which also hands out the unshifted horizontal deltas of every
// word.  (k_fl_tiles keeps its own copy: called from there the function changes its code, 2 388 -> 2 477 instructions for the
// 128 word steps of NW = 16)  p0 / p1: the pattern's planes; r0 / r1: the text base's two bits spread over a
// word; pv / mv: the column's vertical deltas, updated; hp / hn: the horizontal delta carried into the word's first row,
// replaced by the one that leaves its last row; ph / mh: the word's horizontal deltas, unshifted (bit i: row i + 1 of the
// word's 32).
__device__ __forceinline__ void fl_word_step(uint32_t p0, uint32_t p1, uint32_t r0, uint32_t r1, uint32_t &pv, uint32_t &mv,
                                             uint32_t &hp, uint32_t &hn, uint32_t &ph, uint32_t &mh)
{
    const uint32_t Eq = ~(p0 ^ r0) & ~(p1 ^ r1);
    const uint32_t Xv = Eq | mv, Eqh = Eq | hn;
    const uint32_t Xh = (((Eqh & pv) + pv) ^ pv) | Eqh;
    ph = mv | ~(Xh | pv); mh = pv & Xh;
    const uint32_t hp2 = ph >> 31, hn2 = mh >> 31;
    const uint32_t sp = (ph << 1) | hp, sm = (mh << 1) | hn;
    pv = sm | ~(Xv | sp);
    mv = sp & Xv;
    hp = hp2; hn = hn2;
}

// a base as pfl.h numbers it, a c g t -> 0 1 2 3, from fl_code's 0 1 3 2
__device__ __forceinline__ uint32_t fl_acgt(int code) { return (uint32_t)(code ^ (code >> 1)); }

// One wave per tile {backbone, first member, end of the backbone's members}; lane l has member first + l.  The members are
// sorted by backbone, a backbone is one more window in mode 0 (bwin / bfl; its a = its blocks, its need = blocks * 32 * NW),
// and the wave walks its blocks in this one launch: a lane's cursor, its alive flag and its sums never leave its registers.
// Per block the column step is k_fl_tiles's over exactly NW full words and m + m / 4 columns for every lane; besides it every
// column stores, per word, Pv after the update (bit x - 1: D(x,y) = D(x-1,y) + 1, "up") and the unshifted Ph (bit x - 1:
// D(x,y) = D(x,y-1) + 1, "left") to the wave's scratch, [column][plane][word][lane]: 256 contiguous bytes a store.  The
// traceback is then the lane's own loop over what it stored itself (the same thread's stores and loads: program order holds).
// A position's byte is complete when the path leaves its row, so four positions go out as one word.
template <int NW>
__global__ __launch_bounds__(64) void k_fl_place(const unsigned char *__restrict__ win, const FlFlank *__restrict__ fl,
                                                 const unsigned char *__restrict__ bwin, const FlFlank *__restrict__ bfl,
                                                 const int4 *__restrict__ tiles, int max_permille, uint32_t *scratch,
                                                 unsigned char *ops, long long ostride, int *__restrict__ blocks,
                                                 int *__restrict__ used, int *__restrict__ dsum)
{
    constexpr int M = 32 * NW, COLS = M + M / 4;
    const int lane = threadIdx.x;
    const int4 tile = tiles[blockIdx.x];
    const FlFlank p = bfl[tile.x];
    const int js = tile.y + lane;
    const bool have = js < tile.z;
    const FlFlank t = fl[have ? js : tile.y];
    uint32_t *const scr = scratch + (size_t)blockIdx.x * ((size_t)COLS * 2 * NW * 64) + lane;
    uint32_t *const row = (uint32_t *)(ops + (size_t)(have ? js : tile.y) * (size_t)ostride);
    int s = 0, voted = 0, sum = 0;
    bool alive = have;
    for (int b = 0; b < p.a; ++b) {
        alive = alive && t.need - s >= M;                   // |M| - s < block: the member stops
        if (!__any(alive)) break;
        uint32_t P0[NW], P1[NW];
#pragma unroll
        for (int h = 0; h < (NW + 1) / 2; ++h) {
            const int x = h * 64 + lane;
            const int code = x < M ? fl_code(bwin, p, b * M + x) : 0;
            const unsigned long long b0 = __ballot(code & 1), b1 = __ballot(code & 2);
            P0[2 * h] = (uint32_t)b0; P1[2 * h] = (uint32_t)b1;
            if (2 * h + 1 < NW) { P0[2 * h + 1] = (uint32_t)(b0 >> 32); P1[2 * h + 1] = (uint32_t)(b1 >> 32); }
        }
        const int tl = min(t.need - s, COLS);               // |T| (of a lane that is alive: >= M)
        uint32_t Pv[NW], Mv[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) { Pv[w] = ~0u; Mv[w] = 0u; }
        int score = M, best = M, ystar = 0;                 // D(m,0) = m
        uint32_t *sp = scr;
        // every lane steps all COLS columns (a multiple of FL_AHEAD); past |T| it fetches its last base again, and a lane that
        // has stopped fetches nothing: what either computes there is never looked at
        for (int y0 = 0; y0 < COLS; y0 += FL_AHEAD) {
            int cs[FL_AHEAD];
#pragma unroll
            for (int k = 0; k < FL_AHEAD; ++k) cs[k] = alive ? fl_code(win, t, s + min(y0 + k, tl - 1)) : 0;
#pragma unroll
            for (int k = 0; k < FL_AHEAD; ++k) {
                const int cur = cs[k];
                const uint32_t r0 = (cur & 1) ? ~0u : 0u, r1 = (cur & 2) ? ~0u : 0u;
                uint32_t hp = 1u, hn = 0u, tp = 0u, tn = 0u;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    uint32_t Ph, Mh;
                    fl_word_step(P0[w], P1[w], r0, r1, Pv[w], Mv[w], hp, hn, Ph, Mh);
                    sp[w * 64] = Pv[w];
                    sp[(NW + w) * 64] = Ph;
                    if (w == NW - 1) { tp = Ph; tn = Mh; }
                }
                sp += 2 * NW * 64;
                score += (int)(tp >> 31) - (int)(tn >> 31);     // D(m, y0 + k + 1): row m is bit 31 of the last word
                if (y0 + k < tl && score < best) { best = score; ystar = y0 + k + 1; }   // (<: the first minimum)
            }
        }
        alive = alive && 1000LL * best <= (long long)max_permille * M;
        if (alive) {
            int x = M, y = ystar, at_y = -1, at_w = -1;
            uint32_t pv = 0u, ph = 0u, ins = 0u, word = 0u;
            while (x > 0) {                                 // (at x = 0 only left steps remain, and they vote for nothing)
                int step = 0;                               // 0 up, 1 left, 2 diagonal; column 0 is all "up"
                if (y > 0) {
                    const int w = (x - 1) >> 5;
                    if (y != at_y || w != at_w) {
                        const uint32_t *q = scr + ((size_t)(y - 1) * 2 * NW + w) * 64;
                        pv = q[0]; ph = q[NW * 64];
                        at_y = y; at_w = w;
                    }
                    const uint32_t bit = 1u << ((x - 1) & 31);
                    step = (pv & bit) ? 0 : (ph & bit) ? 1 : 2;
                }
                if (step == 1) { ins = 1u + fl_acgt(fl_code(win, t, s + y - 1)); --y; continue; }
                const uint32_t byte = (step == 0 ? 4u : fl_acgt(fl_code(win, t, s + y - 1))) | (ins << 4);
                ins = 0u;
                --x;
                word |= byte << (8 * (x & 3));
                if ((x & 3) == 0) { row[(b * M + x) >> 2] = word; word = 0u; }
                if (step == 2) --y;
            }
            s += ystar; sum += best; ++voted;
        }
    }
    if (have) { blocks[js] = voted; used[js] = s; dsum[js] = sum; }
}

// one thread per (backbone, position): the votes of the backbone's members, which are neighbours in ops after the sort, so
// the threads of a wave read 64 neighbouring bytes of one member's row at a time
__global__ __launch_bounds__(256) void k_fl_votes(const unsigned char *__restrict__ ops, long long ostride, const int4 *__restrict__ cl,
                                                  unsigned char *__restrict__ sym, unsigned char *__restrict__ ins,
                                                  int *__restrict__ voters)
{
    const int4 c = cl[blockIdx.y];                          // {first member, end, positions}
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.z) return;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    for (int k = c.x; k < c.y; ++k) {
        const int o = ops[(size_t)k * (size_t)ostride + i], lo = o & 15, hi = o >> 4;
        n0 += lo == 0; n1 += lo == 1; n2 += lo == 2; n3 += lo == 3; n4 += lo == 4;
        i0 += hi == 1; i1 += hi == 2; i2 += hi == 3; i3 += hi == 4;
    }
    int s = 0, top = n0;                                    // the first largest of a c g t gap
    if (n1 > top) { s = 1; top = n1; }
    if (n2 > top) { s = 2; top = n2; }
    if (n3 > top) { s = 3; top = n3; }
    if (n4 > top) { s = 4; top = n4; }
    const int v = n0 + n1 + n2 + n3 + n4;
    int e = 0, etop = i0;
    if (i1 > etop) { e = 1; etop = i1; }
    if (i2 > etop) { e = 2; etop = i2; }
    if (i3 > etop) { e = 3; etop = i3; }
    const size_t at = (size_t)blockIdx.y * (size_t)ostride + i;
    sym[at] = (unsigned char)s;
    ins[at] = (unsigned char)(2 * (i0 + i1 + i2 + i3) > v ? 1 + e : 0);
    voters[at] = v;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <class T> struct FlBuf {   // a device buffer of the context that only grows
    T *p = nullptr;
    size_t cap = 0;
    bool room(size_t n)
    {
        if (n <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) { p = nullptr; return false; }
        cap = n;
        return true;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct pfl_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    FlBuf<unsigned char> win;
    FlBuf<FlFlank> fl;
    FlBuf<int2> tiles;
    FlBuf<int> dist;
    unsigned long long cells = 0;
    double kernel_ms = 0.0;
    // the placements (pfl_place, pfl_consensus)
    FlBuf<unsigned char> bwin, ops, sym, ins;
    FlBuf<FlFlank> bfl;
    FlBuf<int4> ptiles, pcl;
    FlBuf<int> pstat, voters;
    FlBuf<uint32_t> scratch;
    long long scratch_limit = FL_SCRATCH_DEFAULT;
    unsigned long long place_cells = 0;
    double place_ms = 0.0, votes_ms = 0.0;
};

static int create(pfl_ctx **out, int device)
{
    if (!out || device < 0) return PWR_ERR_ARG;
    pfl_ctx *c = new (std::nothrow) pfl_ctx();
    if (!c) return PWR_ERR_NOMEM;
    c->device = device;                                     // (the device is first touched by the first call that has pairs)
    *out = c;
    return PWR_OK;
}

static int open_device(pfl_ctx *c)
{
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (!c->stream && hipStreamCreate(&c->stream) != hipSuccess) { c->stream = nullptr; return PWR_ERR_DEVICE; }
    if (!c->e0 && hipEventCreate(&c->e0) != hipSuccess) { c->e0 = nullptr; return PWR_ERR_DEVICE; }
    if (!c->e1 && hipEventCreate(&c->e1) != hipSuccess) { c->e1 = nullptr; return PWR_ERR_DEVICE; }
    return PWR_OK;
}

extern "C" int pfl_create(pfl_ctx **out, int device)
{
    return abi_guard([&] { return create(out, device); });
}

extern "C" void pfl_destroy(pfl_ctx *c)
{
    if (!c) return;
    if (c->stream) (void)hipSetDevice(c->device);
    c->win.release(); c->fl.release(); c->tiles.release(); c->dist.release();
    c->bwin.release(); c->ops.release(); c->sym.release(); c->ins.release(); c->bfl.release(); c->ptiles.release();
    c->pcl.release(); c->pstat.release(); c->voters.release(); c->scratch.release();
    if (c->e0) (void)hipEventDestroy(c->e0);
    if (c->e1) (void)hipEventDestroy(c->e1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int pfl_get_stats(pfl_ctx *c, unsigned long long *cells, double *kernel_ms)
{
    if (!c) return PWR_ERR_ARG;
    if (cells) *cells = c->cells;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    return PWR_OK;
}

// the kernel takes a base's code from two bits of its character: anything else would silently alias one of the four
static inline bool fl_is_base(char ch)
{
    switch (ch) { case 'a': case 'c': case 'g': case 't': case 'A': case 'C': case 'G': case 'T': return true; default: return false; }
}

template <int NW>
static void launch_tiles(int nw, unsigned ntiles, hipStream_t st, const unsigned char *win, const FlFlank *fl, const int2 *tiles, int ns, int *dist)
{
    if (nw == NW) { hipLaunchKernelGGL((k_fl_tiles<NW>), dim3(ntiles), dim3(64), 0, st, win, fl, tiles, ns, dist); return; }
    if constexpr (NW < FL_MAXW) launch_tiles<NW + 1>(nw, ntiles, st, win, fl, tiles, ns, dist);
}

static int distances(pfl_ctx *c, int n, const char *bases, const long long *off, const int *piece, const int *mode, int reach,
                     int min_len, int *len_out, int *dist_out)
{
    if (!c || n < 0 || (n && (!bases || !off || !piece || !mode || !len_out || !dist_out))) return PWR_ERR_ARG;
    if (reach < 1 || reach > PFL_MAX_REACH || min_len < 1 || n > PFL_MAX_FLANKS) return PWR_ERR_RANGE;
    for (int k = 0; k < n; ++k) {
        if (piece[k] < 0 || mode[k] < 0 || mode[k] > 3) return PWR_ERR_ARG;
        const long long l = off[piece[k] + 1] - off[piece[k]];
        if (l < 0 || l > 0x7fffffff) return l < 0 ? PWR_ERR_ARG : PWR_ERR_RANGE;
        len_out[k] = (int)l;
    }
    for (int k = 0; k < n; ++k) {
        const char *b = bases + off[piece[k]];
        for (int x = 0; x < len_out[k]; ++x) if (!fl_is_base(b[x])) return PWR_ERR_INPUT;
    }
    std::fill(dist_out, dist_out + (size_t)n * n, -1);
    std::vector<int> order;
    for (int k = 0; k < n; ++k) if (len_out[k] >= min_len) { order.push_back(k); dist_out[(size_t)k * n + k] = 0; }
    const int ns = (int)order.size();
    if (ns < 2) return PWR_OK;
    auto a_of = [&](int k) { return std::min(len_out[k], reach); };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a_of(x) < a_of(y); });   // (stable: the index breaks ties)
    // the window of every flank, packed: the bytes nearest to the boundary, in the piece's own orientation
    const int wide = reach + reach / 4;
    std::vector<FlFlank> hf((size_t)ns);
    std::vector<unsigned char> win;
    win.reserve((size_t)ns * wide);
    for (int s = 0; s < ns; ++s) {
        const int k = order[s], need = std::min(len_out[k], wide);
        const char *b = bases + off[piece[k]] + ((mode[k] & 1) ? len_out[k] - need : 0);
        hf[s].woff = (int)win.size(); hf[s].need = need; hf[s].a = a_of(k); hf[s].mode = mode[k];
        win.insert(win.end(), b, b + need);
    }
    // tiles: pattern s against the texts s + 1 .. ns - 1 in runs of 64, grouped by the pattern's word count (ascending with s)
    std::vector<int2> tiles;
    int first_of[FL_MAXW + 2];
    int nw_at = 0;
    for (int s = 0; s + 1 < ns; ++s) {
        const int nw = (hf[s].a + 31) / 32, m = hf[s].a;
        while (nw_at < nw) first_of[++nw_at] = (int)tiles.size();
        for (int t = s + 1; t < ns; t += 64) tiles.push_back(make_int2(s, t));
        for (int t = s + 1; t < ns; ++t) c->cells += (unsigned long long)m * (unsigned long long)std::min(hf[t].need, m + m / 4);
    }
    while (nw_at < FL_MAXW + 1) first_of[++nw_at] = (int)tiles.size();
    if (const int rc = open_device(c)) return rc;
    if (!c->win.room(win.size()) || !c->fl.room(hf.size()) || !c->tiles.room(tiles.size()) || !c->dist.room((size_t)ns * ns)) return PWR_ERR_NOMEM;
    HIPC(hipMemcpyAsync(c->win.p, win.data(), win.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->fl.p, hf.data(), sizeof(FlFlank) * hf.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->tiles.p, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipEventRecord(c->e0, c->stream));
    for (int nw = 1; nw <= FL_MAXW; ++nw) {
        const int lo = first_of[nw], hi = first_of[nw + 1];
        if (hi > lo) launch_tiles<1>(nw, (unsigned)(hi - lo), c->stream, c->win.p, c->fl.p, c->tiles.p + lo, ns, c->dist.p);
        HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(c->e1, c->stream));
    std::vector<int> ds((size_t)ns * ns);
    HIPC(hipMemcpyAsync(ds.data(), c->dist.p, sizeof(int) * ds.size(), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->kernel_ms += ms;
    for (int s = 0; s < ns; ++s)
        for (int t = s + 1; t < ns; ++t) {
            const int i = order[s], j = order[t], d = ds[(size_t)s * ns + t];
            dist_out[(size_t)i * n + j] = d; dist_out[(size_t)j * n + i] = d;
        }
    return PWR_OK;
}

extern "C" int pfl_distances(pfl_ctx *c, int n, const char *bases, const long long *off, const int *piece, const int *mode, int reach,
                             int min_len, int *len_out, int *dist_out)
{
    return abi_guard([&] { return distances(c, n, bases, off, piece, mode, reach, min_len, len_out, dist_out); });
}

// ---------------------------------------------------------------------------------------------
// host side of the placements
// ---------------------------------------------------------------------------------------------
struct FlSeq { const char *p; int len; };   // a backbone on the host

struct FlPlacement {                // the members of one call, sorted by backbone, and this round's backbones
    int ns = 0, nb = 0, block = 0, extent = 0, ntiles = 0;
    std::vector<int> order;         // sorted position -> flank
    std::vector<int> first;         // [nb + 1]: backbone j's members are the sorted positions first[j] .. first[j + 1]
    std::vector<int> use;           // [nb]: the bases of backbone j that are used, blocks * block (0: nothing to place)
    long long ostride = 0;          // bytes of a row of ops on the device: the largest use
};

// the arguments pfl_place and pfl_consensus share; len[k] = the length of flank k's piece
static int check_flanks(int n, const char *bases, const long long *off, const int *piece, const int *mode, const int *group,
                        int block, int extent, int max_permille, std::vector<int> &len)
{
    if (n < 0 || (n && (!bases || !off || !piece || !mode || !group))) return PWR_ERR_ARG;
    if (block < 32 || block > PFL_MAX_REACH || block % 32 || extent < block || extent > PFL_MAX_EXTENT || n > PFL_MAX_FLANKS)
        return PWR_ERR_RANGE;
    if (max_permille < 0) return PWR_ERR_ARG;
    len.assign((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        if (piece[k] < 0 || mode[k] < 0 || mode[k] > 3) return PWR_ERR_ARG;
        const long long l = off[piece[k] + 1] - off[piece[k]];
        if (l < 0 || l > 0x7fffffff) return l < 0 ? PWR_ERR_ARG : PWR_ERR_RANGE;
        len[k] = (int)l;
    }
    for (int k = 0; k < n; ++k) {
        const char *b = bases + off[piece[k]];
        for (int x = 0; x < len[k]; ++x) if (!fl_is_base(b[x])) return PWR_ERR_INPUT;
    }
    return PWR_OK;
}

// sorts the flanks with cluster[k] >= 0 by (cluster, k) and uploads their windows, once per call
static int members_up(pfl_ctx *c, FlPlacement &P, int n, const char *bases, const long long *off, const int *piece, const int *mode,
                      const std::vector<int> &len, const int *cluster)
{
    P.first.assign((size_t)P.nb + 1, 0);
    for (int k = 0; k < n; ++k) if (cluster[k] >= 0) ++P.first[cluster[k] + 1];
    for (int j = 0; j < P.nb; ++j) P.first[j + 1] += P.first[j];
    P.ns = P.first[P.nb];
    P.order.assign((size_t)P.ns, 0);
    std::vector<int> at(P.first.begin(), P.first.end() - 1);
    for (int k = 0; k < n; ++k) if (cluster[k] >= 0) P.order[at[cluster[k]]++] = k;
    if (P.ns == 0) return PWR_OK;
    const int wide = P.extent + P.extent / 4;
    std::vector<FlFlank> hf((size_t)P.ns);
    std::vector<unsigned char> win;
    for (int s = 0; s < P.ns; ++s) {
        const int k = P.order[s], need = std::min(len[k], wide);
        const char *b = bases + off[piece[k]] + ((mode[k] & 1) ? len[k] - need : 0);
        hf[s].woff = (int)win.size(); hf[s].need = need; hf[s].a = 0; hf[s].mode = mode[k];
        win.insert(win.end(), b, b + need);
    }
    if (const int rc = open_device(c)) return rc;
    if (!c->win.room(std::max<size_t>(win.size(), 1)) || !c->fl.room(hf.size())) return PWR_ERR_NOMEM;
    HIPC(hipMemcpyAsync(c->win.p, win.data(), win.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->fl.p, hf.data(), sizeof(FlFlank) * hf.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return PWR_OK;
}

// this round's backbones: their used blocks as windows in mode 0, the tiles, the member range and positions of every backbone
static int backbones_up(pfl_ctx *c, FlPlacement &P, const std::vector<FlSeq> &seqs, bool votes)
{
    P.use.assign((size_t)P.nb, 0);
    P.ostride = 0; P.ntiles = 0;
    std::vector<FlFlank> hb((size_t)P.nb);
    std::vector<unsigned char> bwin;
    std::vector<int4> tiles, cl((size_t)P.nb);
    for (int j = 0; j < P.nb; ++j) {
        const int blocks = P.first[j + 1] > P.first[j] ? std::min(seqs[j].len, P.extent) / P.block : 0;
        P.use[j] = blocks * P.block;
        hb[j].woff = (int)bwin.size(); hb[j].need = P.use[j]; hb[j].a = blocks; hb[j].mode = 0;
        bwin.insert(bwin.end(), seqs[j].p, seqs[j].p + P.use[j]);
        cl[j] = make_int4(P.first[j], P.first[j + 1], P.use[j], 0);
        if (blocks) for (int t = P.first[j]; t < P.first[j + 1]; t += 64) tiles.push_back(make_int4(j, t, P.first[j + 1], 0));
        P.ostride = std::max<long long>(P.ostride, P.use[j]);
    }
    P.ntiles = (int)tiles.size();
    if (P.ntiles == 0) return PWR_OK;
    if (const int rc = open_device(c)) return rc;
    if (!c->bwin.room(bwin.size()) || !c->bfl.room(hb.size()) || !c->ptiles.room(tiles.size()) || !c->pcl.room(cl.size()) ||
        !c->ops.room((size_t)P.ns * (size_t)P.ostride) || !c->pstat.room((size_t)P.ns * 3))
        return PWR_ERR_NOMEM;
    if (votes && (!c->sym.room((size_t)P.nb * (size_t)P.ostride) || !c->ins.room((size_t)P.nb * (size_t)P.ostride) ||
                  !c->voters.room((size_t)P.nb * (size_t)P.ostride)))
        return PWR_ERR_NOMEM;
    HIPC(hipMemcpyAsync(c->bwin.p, bwin.data(), bwin.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->bfl.p, hb.data(), sizeof(FlFlank) * hb.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->ptiles.p, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->pcl.p, cl.data(), sizeof(int4) * cl.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return PWR_OK;
}

template <int NW>
static void launch_place(int nw, unsigned ntiles, pfl_ctx *c, const int4 *tiles, int max_permille, long long ostride, int ns)
{
    if (nw == NW) {
        hipLaunchKernelGGL((k_fl_place<NW>), dim3(ntiles), dim3(64), 0, c->stream, c->win.p, c->fl.p, c->bwin.p, c->bfl.p, tiles,
                           max_permille, c->scratch.p, c->ops.p, ostride, c->pstat.p, c->pstat.p + ns, c->pstat.p + 2 * (size_t)ns);
        return;
    }
    if constexpr (NW < FL_MAXW) launch_place<NW + 1>(nw, ntiles, c, tiles, max_permille, ostride, ns);
}

// k_fl_place over the tiles, in as many ranges as the scratch asks for; stat[3 * ns] gets blocks, used, dist by sorted position
static int place_run(pfl_ctx *c, const FlPlacement &P, int max_permille, std::vector<int> &stat)
{
    stat.assign((size_t)P.ns * 3, 0);
    if (P.ntiles == 0) return PWR_OK;
    const int nw = P.block / 32, cols = P.block + P.block / 4;
    const size_t words = (size_t)cols * 2 * nw * 64;        // of one tile's scratch
    const long long limit = c->scratch_limit > 0 ? c->scratch_limit : FL_SCRATCH_DEFAULT;
    int per = (int)std::min<long long>(P.ntiles, std::max<long long>(1, limit / (long long)(words * 4)));
    if (const int rc = largest_that_fits(per, [&](int k) { return c->scratch.room((size_t)k * words); })) return rc;
    HIPC(hipMemsetAsync(c->ops.p, 0x0f, (size_t)P.ns * (size_t)P.ostride, c->stream));
    HIPC(hipMemsetAsync(c->pstat.p, 0, sizeof(int) * (size_t)P.ns * 3, c->stream));
    HIPC(hipEventRecord(c->e0, c->stream));
    for (int lo = 0; lo < P.ntiles; lo += per) {            // (one stream: a range has left the scratch before the next takes it)
        launch_place<1>(nw, (unsigned)std::min(per, P.ntiles - lo), c, c->ptiles.p + lo, max_permille, P.ostride, P.ns);
        HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(c->e1, c->stream));
    HIPC(hipMemcpyAsync(stat.data(), c->pstat.p, sizeof(int) * stat.size(), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->place_ms += ms;
    for (int s = 0; s < P.ns; ++s) c->place_cells += (unsigned long long)stat[s] * (unsigned long long)P.block * (unsigned long long)cols;
    return PWR_OK;
}

static int place(pfl_ctx *c, int n, const char *bases, const long long *off, const int *piece, const int *mode, const int *cluster,
                 int nb, const char *bb_bases, const long long *bb_off, int block, int extent, int max_permille, unsigned char *ops,
                 long long stride, int *blocks, int *used, int *dist)
{
    if (!c || nb < 0 || (n > 0 && (!ops || !blocks || !used || !dist)) || (nb && (!bb_bases || !bb_off))) return PWR_ERR_ARG;
    std::vector<int> len;
    if (const int rc = check_flanks(n, bases, off, piece, mode, cluster, block, extent, max_permille, len)) return rc;
    if (nb > PFL_MAX_FLANKS || stride < 0) return PWR_ERR_RANGE;
    FlPlacement P;
    P.nb = nb; P.block = block; P.extent = extent;
    std::vector<FlSeq> seqs((size_t)nb);
    long long most = 0;
    for (int j = 0; j < nb; ++j) {
        const long long l = bb_off[j + 1] - bb_off[j];
        if (l < 0 || l > 0x7fffffff) return l < 0 ? PWR_ERR_ARG : PWR_ERR_RANGE;
        seqs[j].p = bb_bases + bb_off[j]; seqs[j].len = (int)l;
        most = std::max<long long>(most, std::min<long long>(l, extent) / block * block);
    }
    for (int k = 0; k < n; ++k) if (cluster[k] < -1 || cluster[k] >= nb) return PWR_ERR_ARG;
    if (stride < most) return PWR_ERR_RANGE;
    for (int j = 0; j < nb; ++j) for (int x = 0; x < seqs[j].len; ++x) if (!fl_is_base(seqs[j].p[x])) return PWR_ERR_INPUT;
    if (n) {
        std::memset(ops, 0x0f, (size_t)n * (size_t)stride);
        std::fill(blocks, blocks + n, 0); std::fill(used, used + n, 0); std::fill(dist, dist + n, 0);
    }
    if (const int rc = members_up(c, P, n, bases, off, piece, mode, len, cluster)) return rc;
    if (P.ns == 0) return PWR_OK;
    if (const int rc = backbones_up(c, P, seqs, false)) return rc;
    if (P.ntiles == 0) return PWR_OK;
    std::vector<int> stat;
    if (const int rc = place_run(c, P, max_permille, stat)) return rc;
    std::vector<unsigned char> rows((size_t)P.ns * (size_t)P.ostride);
    HIPC(hipMemcpy(rows.data(), c->ops.p, rows.size(), hipMemcpyDeviceToHost));
    for (int s = 0; s < P.ns; ++s) {
        const int k = P.order[s];
        std::memcpy(ops + (size_t)k * (size_t)stride, rows.data() + (size_t)s * (size_t)P.ostride, (size_t)P.use[cluster[k]]);
        blocks[k] = stat[s]; used[k] = stat[(size_t)P.ns + s]; dist[k] = stat[2 * (size_t)P.ns + s];
    }
    return PWR_OK;
}

extern "C" int pfl_place(pfl_ctx *c, int n, const char *bases, const long long *off, const int *piece, const int *mode,
                         const int *cluster, int nb, const char *bb_bases, const long long *bb_off, int block, int extent,
                         int max_permille, unsigned char *ops, long long stride, int *blocks, int *used, int *dist)
{
    return abi_guard([&] {
        return place(c, n, bases, off, piece, mode, cluster, nb, bb_bases, bb_off, block, extent, max_permille, ops, stride, blocks,
                     used, dist);
    });
}

extern "C" int pfl_set_scratch_limit(pfl_ctx *c, long long bytes)
{
    if (!c) return PWR_ERR_ARG;
    c->scratch_limit = bytes > 0 ? bytes : FL_SCRATCH_DEFAULT;
    return PWR_OK;
}

extern "C" int pfl_get_place_stats(pfl_ctx *c, unsigned long long *cells, double *place_ms, double *votes_ms)
{
    if (!c) return PWR_ERR_ARG;
    if (cells) *cells = c->place_cells;
    if (place_ms) *place_ms = c->place_ms;
    if (votes_ms) *votes_ms = c->votes_ms;
    return PWR_OK;
}

// k_fl_votes over every backbone's positions, and its three outputs [nb][ostride] to the host
static int votes_run(pfl_ctx *c, const FlPlacement &P, std::vector<unsigned char> &sym, std::vector<unsigned char> &ins,
                     std::vector<int> &voters)
{
    const size_t cells = (size_t)P.nb * (size_t)P.ostride;
    sym.assign(cells, 0); ins.assign(cells, 0); voters.assign(cells, 0);
    if (P.ntiles == 0) return PWR_OK;
    HIPC(hipEventRecord(c->e0, c->stream));
    hipLaunchKernelGGL(k_fl_votes, dim3((unsigned)((P.ostride + 255) / 256), (unsigned)P.nb), dim3(256), 0, c->stream, c->ops.p,
                       P.ostride, c->pcl.p, c->sym.p, c->ins.p, c->voters.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->e1, c->stream));
    // (a position past a backbone's use is not written on the device and not read on the host)
    HIPC(hipMemcpyAsync(sym.data(), c->sym.p, cells, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(ins.data(), c->ins.p, cells, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(voters.data(), c->voters.p, sizeof(int) * cells, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->votes_ms += ms;
    return PWR_OK;
}

static int consensus(pfl_ctx *c, int n, const char *bases, const long long *off, const int *piece, const int *mode, const int *label,
                     int block, int extent, int max_permille, int min_depth, int rounds, pfl_consensus_result *out)
{
    if (!out) return PWR_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    if (!c) return PWR_ERR_ARG;
    std::vector<int> len;
    if (const int rc = check_flanks(n, bases, off, piece, mode, label, block, extent, max_permille, len)) return rc;
    if (rounds < 1) return PWR_ERR_RANGE;
    if (min_depth < 1) return PWR_ERR_ARG;
    for (int k = 0; k < n; ++k) if (label[k] < -1) return PWR_ERR_ARG;
    std::vector<int> names;
    for (int k = 0; k < n; ++k) if (label[k] >= 0) names.push_back(label[k]);
    std::sort(names.begin(), names.end());
    names.erase(std::unique(names.begin(), names.end()), names.end());
    const int nb = (int)names.size();
    std::vector<int> cluster((size_t)n, -1), members((size_t)nb, 0), backbone((size_t)nb, -1);
    for (int k = 0; k < n; ++k) {
        if (label[k] < 0 || len[k] < block) continue;
        const int j = (int)(std::lower_bound(names.begin(), names.end(), label[k]) - names.begin());
        cluster[k] = j; ++members[j];
        if (backbone[j] < 0 || len[k] > len[backbone[j]]) backbone[j] = k;          // (>: the lowest index among the longest)
    }
    // round 1's backbones: the anchored sequence of the longest member, as far as extent reaches
    std::vector<std::vector<char>> seq((size_t)nb);
    std::vector<std::vector<int>> depth((size_t)nb);
    std::vector<char> done((size_t)nb, 0);
    for (int j = 0; j < nb; ++j) {
        const int k = backbone[j];
        if (k < 0) { done[j] = 1; continue; }
        const char *b = bases + off[piece[k]];
        const int l = std::min(len[k], extent);
        seq[j].resize((size_t)l);
        for (int y = 0; y < l; ++y) {
            const int ch = (unsigned char)b[(mode[k] & 1) ? len[k] - 1 - y : y];
            const int code = ((ch >> 1) & 3) ^ (mode[k] & 2);                      // fl_code's: a c g t -> 0 1 3 2
            seq[j][y] = "acgt"[code ^ (code >> 1)];
        }
    }
    FlPlacement P;
    P.nb = nb; P.block = block; P.extent = extent;
    if (const int rc = members_up(c, P, n, bases, off, piece, mode, len, cluster.data())) return rc;
    std::vector<FlSeq> seqs((size_t)nb);
    std::vector<int> stat, voters;
    std::vector<unsigned char> sym, ins;
    for (int r = 0; r < rounds; ++r) {
        bool any = false;
        for (int j = 0; j < nb; ++j) {
            seqs[j].p = seq[j].data(); seqs[j].len = done[j] ? 0 : (int)seq[j].size();
            any = any || !done[j];
        }
        if (!any) break;
        if (const int rc = backbones_up(c, P, seqs, true)) return rc;
        if (const int rc = place_run(c, P, max_permille, stat)) return rc;
        if (const int rc = votes_run(c, P, sym, ins, voters)) return rc;
        for (int j = 0; j < nb; ++j) {
            if (done[j]) continue;
            const size_t at = (size_t)j * (size_t)P.ostride;
            std::vector<char> next((size_t)P.use[j] * 2 + 1);
            depth[j].assign((size_t)P.use[j] * 2 + 1, 0);
            const int got = pfl_call(P.use[j], sym.data() + at, ins.data() + at, voters.data() + at, min_depth, next.data(), depth[j].data());
            next.resize((size_t)got); depth[j].resize((size_t)got);
            seq[j].swap(next);
            if (got < block) done[j] = 1;
        }
    }
    std::vector<const char *> sp((size_t)nb + 1, nullptr);
    std::vector<const int *> dp((size_t)nb + 1, nullptr);
    std::vector<int> sl((size_t)nb + 1, 0);
    for (int j = 0; j < nb; ++j) { sp[j] = seq[j].data(); dp[j] = depth[j].data(); sl[j] = backbone[j] < 0 ? 0 : (int)seq[j].size(); }
    return pfl_consensus_pack(nb, names.data(), members.data(), backbone.data(), sp.data(), dp.data(), sl.data(), out);
}

extern "C" int pfl_consensus(pfl_ctx *c, int n, const char *bases, const long long *off, const int *piece, const int *mode,
                             const int *label, int block, int extent, int max_permille, int min_depth, int rounds,
                             pfl_consensus_result *out)
{
    const int rc = abi_guard([&] { return consensus(c, n, bases, off, piece, mode, label, block, extent, max_permille, min_depth, rounds, out); });
    if (rc != PWR_OK && out) pfl_consensus_free(out);
    return rc;
}
