// pla_device.hip -- MI355X (gfx950) implementation of the search behind include/pla.h (pla_open_text, pla_search): a few hundred
// short patterns, each in two orientations, against every contig of an assembly.
//
// The table is semi-global, D(0,y) = 0 and D(x,0) = x with unit costs, and only its last row matters.  A column is two bit
// vectors over the pattern (Pv, Mv), advanced one text base per handful of integer instructions per 32 pattern rows: Myers 1999
// in Hyyro's block form with the carry into row 0 being 0, the step of prc_device.hip and pia_device.hip.  The word step stands
// here a third time (DESIGN 25 says why k_fl_tiles keeps its own): pfl_device.hip is not touched.
//
// Layout: k_fl_tiles's, with the roles of a lane's text changed.  A wave takes a tile = one job (pattern, orientation) and 64
// consecutive chunks of the text, a chunk per lane.  The pattern is wave-uniform: its two bit planes are made by ballots and
// live in scalar registers, ceil(m / 32) words each, the kernel being compiled per word count; a lane keeps Pv and Mv only.  m
// is uniform, so the bit of row m - 1 whose delta moves the score is the same in every lane: no register is indexed at run
// time.  No LDS, no barrier, no atomics: a lane owns its chunk and its slots of the records.
//
// A chunk owns `chunk` consecutive walk columns of one contig (the last chunk of a contig fewer) and never crosses a contig.
// It starts its table m + k walk columns earlier, or at the contig's start, from D(x, .) = x.  That column is an upper bound of
// the true one, and an alignment of cost <= k spans at most m + k text bases and may begin anywhere (D(0, .) = 0), so
// min(D, k + 1) is exact in every owned column.  A lane follows its runs of D(m, y) <= k in registers and writes one 16-byte
// record {y1, y2, minimum, first column of the minimum} per finished run, up to `cap` per chunk, and the exact count; a run
// open at the chunk's last column is closed there and the host joins it to the one that begins the next chunk.  A tile in
// which a chunk has more runs than PLA_RUN_CAP is run again alone with room for the largest count.
//
// The text is on the device as one code per byte (a c g t -> 0 .. 3, everything else 4), in the file's order; a job walks it
// forwards or backwards and complements the codes below 4 as its two bits say.  A lane reads its own bytes, LA_AHEAD per wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#define PWR_STAGE "pla"
#include "dev_util.h"
#include "pla.h"

#define LA_MAXW (PLA_MAX_REACH / 32)
#define LA_AHEAD 8                  // text bases fetched per wait
#define LA_CHUNK_DEFAULT 2048
#define LA_TILES_PER_LAUNCH 32768   // 2 Mi lanes: 128 MiB of records at PLA_RUN_CAP and 8 MiB of counts
#define LA_RERUN_BYTES (256LL << 20)   // records of one re-run launch at most (a single tile always goes)
static_assert(LA_MAXW * 32 == PLA_MAX_REACH, "PLA_MAX_REACH is what the widest kernel holds");

struct LaJob {
    int qoff;                       // offset of the job's rows Q in the packed pattern codes
    int m;                          // rows
    int k;                          // floor(max_permille * m / 1000)
    int flags;                      // bit 0: the walk runs from the contig's last base down; bit 1: complemented
};

struct LaChunk {
    long long toff;                 // offset of the chunk's contig in the text
    int len;                        // L_c
    int y0;                         // the chunk owns the walk columns y0 + 1 .. y0 + n (W[y0 .. y0 + n))
    int n;
    int contig;
};

// one wave per tile {job, first chunk}; lane l has chunk first + l
template <int NW>
__global__ __launch_bounds__(64) void k_la_search(const unsigned char *__restrict__ text, const unsigned char *__restrict__ pat,
                                                  const LaJob *__restrict__ jobs, const LaChunk *__restrict__ chunks, int nchunks,
                                                  const int2 *__restrict__ tiles, int cap, int4 *__restrict__ rec,
                                                  int *__restrict__ count)
{
    const int lane = threadIdx.x;
    const int2 tile = tiles[blockIdx.x];
    const LaJob job = jobs[tile.x];
    const int m = job.m, kk = job.k;                        // 32 * (NW - 1) < m <= 32 * NW
    // the pattern's planes: bit x of plane 0/1 = bit 0/1 of the code of row x (rows past m - 1 hold an 'a': what a row above
    // m - 1 does never reaches the rows below it)
    uint32_t P0[NW], P1[NW];
#pragma unroll
    for (int h = 0; h < (NW + 1) / 2; ++h) {
        const int x = h * 64 + lane;
        const int code = x < m ? pat[job.qoff + x] : 0;
        const unsigned long long b0 = __ballot(code & 1), b1 = __ballot(code & 2);
        P0[2 * h] = (uint32_t)b0; P1[2 * h] = (uint32_t)b1;
        if (2 * h + 1 < NW) { P0[2 * h + 1] = (uint32_t)(b0 >> 32); P1[2 * h + 1] = (uint32_t)(b1 >> 32); }
    }
    const int ci = tile.y + lane;
    const bool have = ci < nchunks;
    const LaChunk ch = chunks[have ? ci : tile.y];          // (a lane without a chunk walks the tile's first one and stores nothing)
    const int start = max(0, ch.y0 - (m + kk));             // the warm-up: m + k columns, or from the contig's start
    const int mine = ch.y0 + ch.n - start;                  // >= 1: a chunk owns at least one column
    int steps = mine;
    for (int o = 32; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o));
    steps = __builtin_amdgcn_readfirstlane(steps);          // (the loop is the wave's, not the lanes')
    const bool back = job.flags & 1, comp = job.flags & 2;
    const unsigned char *const t = text + ch.toff;
    const int bt = (m - 1) & 31;                            // row m - 1 is bit bt of word NW - 1
    uint32_t Pv[NW], Mv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) { Pv[w] = ~0u; Mv[w] = 0u; }   // column `start`: D(x, .) = x
    int score = m;
    int n = 0, y1 = 0, mn = 0, ys = 0;                      // the runs so far; the open run's first column, minimum and its column
    bool open = false;
    int4 *const slot = rec + (size_t)blockIdx.x * (size_t)cap * 64 + lane;
    // LA_AHEAD text bases per fetch.  Past its last column a lane fetches its last base again and steps on; what it computes
    // there is never looked at.  Every index is within start .. y0 + n - 1, inside the contig.
    for (int i0 = 0; i0 < steps; i0 += LA_AHEAD) {
        int cs[LA_AHEAD];
#pragma unroll
        for (int a = 0; a < LA_AHEAD; ++a) {
            const int y = start + min(i0 + a, mine - 1);
            cs[a] = t[back ? ch.len - 1 - y : y];
        }
#pragma unroll
        for (int a = 0; a < LA_AHEAD; ++a) {
            int cur = cs[a];
            const uint32_t known = cur < 4 ? ~0u : 0u;      // code 4 matches nothing
            if (comp) cur = 3 - cur;
            const uint32_t r0 = (cur & 1) ? ~0u : 0u, r1 = (cur & 2) ? ~0u : 0u;
            uint32_t hp = 0u, hn = 0u, tp = 0u, tn = 0u;    // D(0,y+1) - D(0,y) = 0: the pattern may begin anywhere
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t Eq = ~(P0[w] ^ r0) & ~(P1[w] ^ r1) & known;
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
            score += (int)((tp >> bt) & 1u) - (int)((tn >> bt) & 1u);
            const int y = start + i0 + a + 1;               // the column just computed, counted from 1
            if (i0 + a < mine && y > ch.y0) {               // an owned column
                if (score <= kk) {
                    if (!open) { open = true; y1 = y; mn = score; ys = y; }
                    else if (score < mn) { mn = score; ys = y; }   // (<: the first column of the minimum)
                } else if (open) {
                    if (have && n < cap) slot[(size_t)n * 64] = make_int4(y1, y - 1, mn, ys);
                    ++n; open = false;
                }
            }
        }
    }
    if (open) {                                             // closed at the chunk's last column; the host joins it to the next chunk's
        if (have && n < cap) slot[(size_t)n * 64] = make_int4(y1, ch.y0 + ch.n, mn, ys);
        ++n;
    }
    if (have) count[(size_t)blockIdx.x * 64 + lane] = n;
}

// the records of the listed lanes {launch lane, records}, side by side: out[i * cap + r]
__global__ __launch_bounds__(256) void k_la_collect(const int4 *__restrict__ rec, const int2 *__restrict__ list, int nlist, int cap,
                                                    int4 *__restrict__ out)
{
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = at / (size_t)cap;
    const int r = (int)(at % (size_t)cap);
    if (i >= (size_t)nlist) return;
    const int2 e = list[i];
    if (r < e.y) out[at] = rec[((size_t)(e.x >> 6) * (size_t)cap + r) * 64 + (e.x & 63)];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <class T> struct LaBuf {   // a device buffer of the context that only grows
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

struct LaRun { int job, contig, y1, y2, mn, ys; };          // a run of one chunk, or of several once joined
struct LaAgain { int2 tile; int need; };

struct pla_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool is_open = false;
    int chunk = LA_CHUNK_DEFAULT;
    std::vector<long long> off;     // [nc + 1] of the open text
    int chunked_at = 0;             // the chunk size `chunks` was made with (0: not made)
    std::vector<LaChunk> chunks;
    LaBuf<unsigned char> text, pat;
    LaBuf<LaJob> jobs;
    LaBuf<LaChunk> dchunks;
    LaBuf<int2> tiles, list;
    LaBuf<int4> rec, out;
    LaBuf<int> count;
    unsigned long long cells = 0;
    double kernel_ms = 0.0;
};

static int open_device(pla_ctx *c)
{
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (!c->stream && hipStreamCreate(&c->stream) != hipSuccess) { c->stream = nullptr; return PWR_ERR_DEVICE; }
    if (!c->e0 && hipEventCreate(&c->e0) != hipSuccess) { c->e0 = nullptr; return PWR_ERR_DEVICE; }
    if (!c->e1 && hipEventCreate(&c->e1) != hipSuccess) { c->e1 = nullptr; return PWR_ERR_DEVICE; }
    return PWR_OK;
}

extern "C" int pla_create(pla_ctx **out, int device)
{
    return abi_guard([&] {
        if (!out || device < 0) return PWR_ERR_ARG;
        pla_ctx *c = new (std::nothrow) pla_ctx();
        if (!c) return PWR_ERR_NOMEM;
        c->device = device;
        *out = c;
        return PWR_OK;
    });
}

extern "C" void pla_close_text(pla_ctx *c)
{
    if (!c) return;
    if (c->stream) (void)hipSetDevice(c->device);
    c->text.release(); c->dchunks.release();
    c->off.clear(); c->chunks.clear();
    c->chunked_at = 0; c->is_open = false;
}

extern "C" void pla_destroy(pla_ctx *c)
{
    if (!c) return;
    pla_close_text(c);
    c->pat.release(); c->jobs.release(); c->tiles.release(); c->list.release(); c->rec.release(); c->out.release(); c->count.release();
    if (c->e0) (void)hipEventDestroy(c->e0);
    if (c->e1) (void)hipEventDestroy(c->e1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int pla_get_stats(pla_ctx *c, unsigned long long *cells, double *kernel_ms)
{
    if (!c) return PWR_ERR_ARG;
    if (cells) *cells = c->cells;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    return PWR_OK;
}

extern "C" int pla_set_option(pla_ctx *c, const char *name, long long value)
{
    if (!c || !name || std::strcmp(name, "chunk") != 0) return PWR_ERR_ARG;
    if (value < 32 || value > 65536 || value % 4) return PWR_ERR_RANGE;
    c->chunk = (int)value;
    return PWR_OK;
}

static inline int la_code(unsigned char ch)
{
    switch (ch) {
    case 'a': case 'A': return 0;
    case 'c': case 'C': return 1;
    case 'g': case 'G': return 2;
    case 't': case 'T': return 3;
    default: return 4;
    }
}

static int open_text(pla_ctx *c, int nc, const char *bases, const long long *off)
{
    if (!c || nc < 0 || !off || (nc && off[nc] > off[0] && !bases)) return PWR_ERR_ARG;
    for (int j = 0; j < nc; ++j) if (off[j + 1] < off[j]) return PWR_ERR_ARG;
    for (int j = 0; j < nc; ++j) if (off[j + 1] - off[j] > 0x7fffffffLL) return PWR_ERR_RANGE;
    pla_close_text(c);
    const long long total = nc ? off[nc] - off[0] : 0;
    unsigned char table[256];
    for (int b = 0; b < 256; ++b) table[b] = (unsigned char)la_code((unsigned char)b);
    std::vector<unsigned char> codes((size_t)total);
    const unsigned char *src = (const unsigned char *)bases + (total ? off[0] : 0);
    for (long long x = 0; x < total; ++x) codes[(size_t)x] = table[src[x]];
    if (const int rc = open_device(c)) return rc;
    if (!c->text.room((size_t)std::max<long long>(total, 1))) return PWR_ERR_NOMEM;
    if (total) HIPC(hipMemcpyAsync(c->text.p, codes.data(), (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    c->off.resize((size_t)nc + 1);
    for (int j = 0; j <= nc; ++j) c->off[(size_t)j] = off[j] - off[0];
    c->is_open = true;
    return PWR_OK;
}

extern "C" int pla_open_text(pla_ctx *c, int nc, const char *bases, const long long *off)
{
    return abi_guard([&] { return open_text(c, nc, bases, off); });
}

// the chunks of the open text at the context's chunk size, on the host and on the device
static int make_chunks(pla_ctx *c)
{
    if (c->chunked_at == c->chunk) return PWR_OK;
    c->chunks.clear();
    const int nc = (int)c->off.size() - 1;
    for (int j = 0; j < nc; ++j) {
        const int len = (int)(c->off[(size_t)j + 1] - c->off[(size_t)j]);
        for (int y0 = 0; y0 < len; y0 += c->chunk) {
            LaChunk ch;
            ch.toff = c->off[(size_t)j]; ch.len = len; ch.y0 = y0; ch.n = std::min(c->chunk, len - y0); ch.contig = j;
            c->chunks.push_back(ch);
        }
    }
    if (c->chunks.size() > 0x7fffffffULL - 64) return PWR_ERR_RANGE;
    if (!c->chunks.empty()) {
        if (!c->dchunks.room(c->chunks.size())) return PWR_ERR_NOMEM;
        HIPC(hipMemcpyAsync(c->dchunks.p, c->chunks.data(), sizeof(LaChunk) * c->chunks.size(), hipMemcpyHostToDevice, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    c->chunked_at = c->chunk;
    return PWR_OK;
}

template <int NW>
static void launch_search(int nw, unsigned ntiles, pla_ctx *c, int nchunks, int cap)
{
    if (nw == NW) {
        hipLaunchKernelGGL((k_la_search<NW>), dim3(ntiles), dim3(64), 0, c->stream, c->text.p, c->pat.p, c->jobs.p, c->dchunks.p, nchunks,
                           c->tiles.p, cap, c->rec.p, c->count.p);
        return;
    }
    if constexpr (NW < LA_MAXW) launch_search<NW + 1>(nw, ntiles, c, nchunks, cap);
}

// one launch over `tiles` (all of word count nw) with room for `cap` runs per chunk: the runs of every tile in which no chunk
// has more go to `runs`, the other tiles to `again` with their largest count
static int run_tiles(pla_ctx *c, int nw, const std::vector<int2> &tiles, int cap, std::vector<LaRun> &runs, std::vector<LaAgain> &again)
{
    const size_t nt = tiles.size(), lanes = nt * 64;
    const int nchunks = (int)c->chunks.size();
    if (!c->tiles.room(nt) || !c->rec.room(lanes * (size_t)cap) || !c->count.room(lanes)) return PWR_ERR_NOMEM;
    HIPC(hipMemcpyAsync(c->tiles.p, tiles.data(), sizeof(int2) * nt, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(c->count.p, 0, sizeof(int) * lanes, c->stream));
    HIPC(hipEventRecord(c->e0, c->stream));
    launch_search<1>(nw, (unsigned)nt, c, nchunks, cap);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->e1, c->stream));
    std::vector<int> count(lanes);
    HIPC(hipMemcpyAsync(count.data(), c->count.p, sizeof(int) * lanes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->kernel_ms += ms;
    std::vector<int2> list;
    for (size_t t = 0; t < nt; ++t) {
        int most = 0;
        for (int l = 0; l < 64; ++l) most = std::max(most, count[t * 64 + l]);
        if (most > cap) { again.push_back(LaAgain{tiles[t], most}); continue; }
        if (most == 0) continue;
        for (int l = 0; l < 64; ++l) if (count[t * 64 + l]) list.push_back(make_int2((int)(t * 64 + l), count[t * 64 + l]));
    }
    if (list.empty()) return PWR_OK;
    if (runs.size() + list.size() > 2 * (size_t)PLA_MAX_HITS + 64) return PWR_ERR_RANGE;   // (joining halves them at best)
    const size_t slots = list.size() * (size_t)cap;
    if (!c->list.room(list.size()) || !c->out.room(slots)) return PWR_ERR_NOMEM;
    HIPC(hipMemcpyAsync(c->list.p, list.data(), sizeof(int2) * list.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_la_collect, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, c->stream, c->rec.p, c->list.p, (int)list.size(), cap,
                       c->out.p);
    HIPC(hipGetLastError());
    std::vector<int4> got(slots);
    HIPC(hipMemcpyAsync(got.data(), c->out.p, sizeof(int4) * slots, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < list.size(); ++i) {
        const int2 tile = tiles[(size_t)(list[i].x >> 6)];
        const int contig = c->chunks[(size_t)tile.y + (size_t)(list[i].x & 63)].contig;
        for (int r = 0; r < list[i].y; ++r) {
            const int4 e = got[i * (size_t)cap + r];
            runs.push_back(LaRun{tile.x, contig, e.x, e.y, e.z, e.w});
        }
    }
    return PWR_OK;
}

static bool la_is_base(char ch)
{
    switch (ch) { case 'a': case 'c': case 'g': case 't': case 'A': case 'C': case 'G': case 'T': return true; default: return false; }
}

static int fill_hits(const std::vector<int> *cols, pla_hits *out)
{
    const size_t n = cols[0].size();
    int **dst[7] = {&out->pattern, &out->orientation, &out->contig, &out->boundary, &out->lo, &out->hi, &out->distance};
    for (int f = 0; f < 7; ++f) {
        *dst[f] = (int *)std::malloc(sizeof(int) * (n + 1));
        if (!*dst[f]) { pla_hits_free(out); return PWR_ERR_NOMEM; }
        if (n) std::memcpy(*dst[f], cols[f].data(), sizeof(int) * n);
    }
    out->n = (int)n;
    return PWR_OK;
}

static int search(pla_ctx *c, int np, const char *anchored, const long long *aoff, const int *side, int reach, int min_len,
                  int max_permille, pla_hits *out)
{
    if (!out) return PWR_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    if (!c || np < 0 || (np && (!aoff || !side))) return PWR_ERR_ARG;
    for (int p = 0; p < np; ++p) if (side[p] != 0 && side[p] != 1) return PWR_ERR_ARG;
    for (int p = 0; p < np; ++p) if (aoff[p + 1] < aoff[p]) return PWR_ERR_ARG;
    if (np && aoff[np] > aoff[0] && !anchored) return PWR_ERR_ARG;
    if (reach < 1 || reach > PLA_MAX_REACH || max_permille < 0 || max_permille > 500 || min_len < 1 || np > PLA_MAX_PATTERNS) return PWR_ERR_RANGE;
    for (int p = 0; p < np; ++p) if (aoff[p + 1] - aoff[p] > 0x7fffffffLL) return PWR_ERR_RANGE;
    if (np) for (long long x = aoff[0]; x < aoff[np]; ++x) if (!la_is_base(anchored[x])) return PWR_ERR_INPUT;
    if (!c->is_open) return PWR_ERR_UNSUPPORTED;
    // the jobs, by word count: Q[x] = A[m - 1 - x] as codes, once per pattern; the two orientations share it
    std::vector<unsigned char> pat;
    std::vector<LaJob> jobs;
    std::vector<int> job_pattern;
    int first_of[LA_MAXW + 2];
    for (int nw = 1; nw <= LA_MAXW; ++nw) {
        first_of[nw] = (int)jobs.size();
        for (int p = 0; p < np; ++p) {
            const long long len = aoff[p + 1] - aoff[p];
            const int m = (int)std::min<long long>(len, reach);
            if (len < min_len || (m + 31) / 32 != nw) continue;
            const int qoff = (int)pat.size();
            for (int x = 0; x < m; ++x) pat.push_back((unsigned char)la_code((unsigned char)anchored[aoff[p] + (m - 1 - x)]));
            for (int o = 0; o < 2; ++o) {
                jobs.push_back(LaJob{qoff, m, (int)((long long)max_permille * m / 1000), (side[p] != o ? 1 : 0) | (o ? 2 : 0)});
                job_pattern.push_back(p);
            }
        }
    }
    first_of[LA_MAXW + 1] = (int)jobs.size();
    std::vector<int> cols[7];
    if (jobs.empty() || c->off.back() == 0) return fill_hits(cols, out);
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (const int rc = make_chunks(c)) return rc;
    if (!c->pat.room(pat.size()) || !c->jobs.room(jobs.size())) return PWR_ERR_NOMEM;
    HIPC(hipMemcpyAsync(c->pat.p, pat.data(), pat.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->jobs.p, jobs.data(), sizeof(LaJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    const int nchunks = (int)c->chunks.size();
    std::vector<LaRun> runs;
    std::vector<int2> tiles;
    std::vector<LaAgain> again;
    for (int nw = 1; nw <= LA_MAXW; ++nw) {
        again.clear();
        tiles.clear();
        for (int j = first_of[nw]; j < first_of[nw + 1]; ++j) {
            c->cells += (unsigned long long)jobs[(size_t)j].m * (unsigned long long)c->off.back();
            for (int first = 0; first < nchunks; first += 64) {
                tiles.push_back(make_int2(j, first));
                if (tiles.size() == LA_TILES_PER_LAUNCH) {
                    if (const int rc = run_tiles(c, nw, tiles, PLA_RUN_CAP, runs, again)) return rc;
                    tiles.clear();
                }
            }
        }
        if (!tiles.empty()) if (const int rc = run_tiles(c, nw, tiles, PLA_RUN_CAP, runs, again)) return rc;
        // the tiles with a chunk of more runs than the cap, again with room; as many a launch as LA_RERUN_BYTES hold
        for (size_t a = 0; a < again.size();) {
            int need = again[a].need;
            tiles.assign(1, again[a].tile);
            size_t b = a + 1;
            for (; b < again.size(); ++b) {
                const int both = std::max(need, again[b].need);
                if ((long long)(tiles.size() + 1) * 64 * both * (long long)sizeof(int4) > LA_RERUN_BYTES) break;
                need = both; tiles.push_back(again[b].tile);
            }
            std::vector<LaAgain> never;
            if (const int rc = run_tiles(c, nw, tiles, need, runs, never)) return rc;
            if (!never.empty()) return PWR_ERR_INTERNAL;       // (the count was exact)
            a = b;
        }
    }
    // chunking is undone: a run that ends a chunk and the one that begins the next chunk of the same contig are one
    std::sort(runs.begin(), runs.end(), [](const LaRun &a, const LaRun &b) {
        return a.job != b.job ? a.job < b.job : a.contig != b.contig ? a.contig < b.contig : a.y1 < b.y1;
    });
    size_t kept = 0;
    for (size_t i = 0; i < runs.size(); ++i) {
        if (kept && runs[kept - 1].job == runs[i].job && runs[kept - 1].contig == runs[i].contig && runs[kept - 1].y2 + 1 == runs[i].y1) {
            LaRun &r = runs[kept - 1];
            r.y2 = runs[i].y2;
            if (runs[i].mn < r.mn) { r.mn = runs[i].mn; r.ys = runs[i].ys; }   // (<: the walk-first column of the minimum)
        } else runs[kept++] = runs[i];
    }
    runs.resize(kept);
    if (kept > (size_t)PLA_MAX_HITS) return PWR_ERR_RANGE;
    struct Hit { int f[7]; };
    std::vector<Hit> hits(kept);
    for (size_t i = 0; i < kept; ++i) {
        const LaRun &r = runs[i];
        const LaJob &j = jobs[(size_t)r.job];
        const int len = (int)(c->off[(size_t)r.contig + 1] - c->off[(size_t)r.contig]);
        auto b = [&](int y) { return (j.flags & 1) ? len - y : y; };
        hits[i] = Hit{{job_pattern[(size_t)r.job], (j.flags >> 1) & 1, r.contig, b(r.ys), std::min(b(r.y1), b(r.y2)), std::max(b(r.y1), b(r.y2)), r.mn}};
    }
    std::sort(hits.begin(), hits.end(), [](const Hit &a, const Hit &b) {
        for (int f = 0; f < 4; ++f) if (a.f[f] != b.f[f]) return a.f[f] < b.f[f];
        return false;
    });
    for (int f = 0; f < 7; ++f) { cols[f].resize(kept); for (size_t i = 0; i < kept; ++i) cols[f][i] = hits[i].f[f]; }
    return fill_hits(cols, out);
}

extern "C" int pla_search(pla_ctx *c, int np, const char *anchored, const long long *aoff, const int *side, int reach, int min_len,
                          int max_permille, pla_hits *out)
{
    const int rc = abi_guard([&] { return search(c, np, anchored, aoff, side, reach, min_len, max_permille, out); });
    if (rc != PWR_OK && out) pla_hits_free(out);
    return rc;
}
