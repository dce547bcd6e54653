// pfl_device.hip -- MI355X (gfx950) implementation of the flank distances behind include/pfl.h (pfl_distances).
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
