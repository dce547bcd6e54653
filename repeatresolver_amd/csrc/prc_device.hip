// prc_device.hip -- MI355X (gfx950) implementation of the ReadCutter's hot loop behind include/prc.h.
//
// Reference: PhilippBongartz/RepeatResolver, ReadCutter.c ("RC:"), Occurrence (RC:491-520): the semi-global edit distance of a
// template piece (length len) into a read, unit costs, M(x,-1) = x + 1, M(-1,y) = 0, and of that matrix only the last row
// M(len-1, y) is used, by the scan of RC:525-567, which looks only at the columns whose score is below the cutoff.
//
// Unit costs make neighbouring cells differ by -1, 0 or +1, so a column of the matrix is kept as two bit vectors over the piece
// (Pv: M(x,y) - M(x-1,y) = +1, Mv: = -1) and advanced one read base per handful of integer instructions per 32 piece rows
// (Myers 1999, in the block form of Hyyro 2001 with a carried-in horizontal delta per word; the same step as pia_device.hip).
// The last row's score starts at len (column -1) and moves by the horizontal delta leaving bit len-1.
//
// Layout: a group of G lanes (a power of two, G * WPL words >= ceil(len / 32)) owns one job = (read, piece); lane l of the
// group holds the words [l * WPL, (l + 1) * WPL) in registers and works on read base y = step - l, so the delta leaving its
// last word reaches lane l + 1 one step later through a lane shift -- no LDS, no barrier.  With len <= 2048 a wave runs 64 / G
// jobs side by side (len = 500, the default's piece: 16 lanes, four jobs per wave).  The jobs are sorted longest read first,
// so the jobs that share a wave have similar lengths and the longest start first.
//
// Output: the lane that holds bit len-1 turns its scores into runs of consecutive columns with score < cutoff, one int4 each
// {first column, last column, minimum, largest column holding the minimum}: all that the scan needs (prc_scan_runs).  A job
// has room for `cap` runs; it always counts all of them, and the host re-runs every job whose count exceeds its room with
// exactly that much room, so nothing is dropped.
//
// Both strands (prc_occurrences_strands, prc_cut_strands): a job carries its strand.  Base y of rc(read) is the complement of
// read[L-1-y], and with the codes a c g t -> 0 1 3 2 the complement flips bit 1 of the code, bit 2 of the character.  A reverse
// job therefore differs from a forward one only where the kernel loads a base: it walks the read from its far end and flips
// that bit.  Its columns y, and so its runs and positions, are in the coordinates of rc(read).  The kernels that look at a
// job's strand are instances of their own (BOTH): prc_occurrences and prc_cut run the ones that do not, the code they always ran.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#define PWR_STAGE "prc"
#include "dev_util.h"
#include "prc.h"

#define RC_MAXWPL 20                // PRC_MAX_PART / (64 lanes x 32 bits)
static_assert(RC_MAXWPL * 64 * 32 == PRC_MAX_PART, "PRC_MAX_PART is what the widest kernel holds");

struct RcJob {
    long long boff;                 // offset of the read's bases in the call's array
    long long roff;                 // offset (int4) of its room for runs
    int L;                          // read length
    int pat;                        // piece: 0 = piece 0, 1 = piece parts-1
    int cap;                        // runs it has room for
    int strand;                     // 1: the job maps the piece into rc(read), read from the same bases backwards
};

// one group of G lanes per job; 64 / G groups per wave (one wave per block)
template <int WPL, bool BOTH>
__global__ __launch_bounds__(64) void k_rc_rows(const uint32_t *__restrict__ planes, int nwords, int len, int cutoff,
                                                const char *__restrict__ bases, const RcJob *__restrict__ jobs,
                                                const int *__restrict__ order, int njobs, int G, int4 *__restrict__ runs,
                                                int *__restrict__ counts)
{
    const int lane = threadIdx.x, lg = lane & (G - 1);
    const int slot = blockIdx.x * (64 / G) + lane / G;
    const bool have = slot < njobs;
    const int jid = have ? order[slot] : 0;
    const RcJob jb = jobs[jid];
    const int L = have ? jb.L : 0;
    const int wt = (len - 1) >> 5, bt = (len - 1) & 31;   // word and bit of piece row len-1
    const int toplane = wt / WPL;                          // the group's lane that holds it
    const int tw = wt - lg * WPL;                          // its word within that lane (meaningful there only)
    // piece planes: bit y of plane 0/1 = bit 0/1 of the base code of piece row y, plane 2 = row y exists in the template
    // (bytes past the template's end match nothing)
    const uint32_t *pl = planes + (size_t)jb.pat * 3 * nwords;
    uint32_t P0[WPL], P1[WPL], V[WPL], Pv[WPL], Mv[WPL];
#pragma unroll
    for (int w = 0; w < WPL; ++w) {
        const int g = lg * WPL + w;
        const bool in = g < nwords;
        P0[w] = in ? pl[g] : 0u; P1[w] = in ? pl[nwords + g] : 0u; V[w] = in ? pl[2 * nwords + g] : 0u;
        Pv[w] = ~0u; Mv[w] = 0u;                            // column -1: M(x,-1) - M(x-1,-1) = +1
    }
    // a reverse job walks the read from its far end, base y at read[-y], with the complement's bit flipped
    const int strand = BOTH ? jb.strand : 0;
    const char *read = bases + jb.boff + (strand ? L - 1 : 0);
    const int dir = strand ? -1 : 1, flip = strand << 2;
    // every group runs L + toplane steps; the wave runs its longest group's
    int steps = L > 0 ? L + toplane : 0;
    for (int o = 32; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o));
    const bool active = lg <= toplane;
    int score = len, nrun = 0, inrun = 0, lo = 0, mn = 0, ey = 0;
    int msg = 0;                                            // horizontal delta leaving the lane's last word: +1 (bit 0), -1 (bit 1)
    int ch = (active && L > 0 && lg == 0) ? read[0] ^ flip : 0;   // base of the next step, loaded one step ahead
    for (int tau = 0; tau < steps; ++tau) {
        int m = __shfl_up(msg, 1);
        if (lg == 0) m = 0;                                 // M(-1,y) - M(-1,y-1) = 0: a free start anywhere in the read
        const int y = tau - lg;
        const int c = ch;
        if (active && y + 1 >= 0 && y + 1 < L) ch = read[dir * (y + 1)] ^ flip;
        if (active && y >= 0 && y < L) {
            const uint32_t r0 = (c >> 1) & 1 ? ~0u : 0u, r1 = (c >> 2) & 1 ? ~0u : 0u;   // a c g t -> 0 1 3 2
            uint32_t hp = m & 1, hn = (m >> 1) & 1, tp = 0, tn = 0;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                const uint32_t Eq = ~(P0[w] ^ r0) & ~(P1[w] ^ r1) & V[w];
                const uint32_t Xv = Eq | Mv[w], Eqh = Eq | hn;
                const uint32_t Xh = (((Eqh & Pv[w]) + Pv[w]) ^ Pv[w]) | Eqh;
                uint32_t Ph = Mv[w] | ~(Xh | Pv[w]), Mh = Pv[w] & Xh;
                if (w == tw) { tp = Ph; tn = Mh; }
                const uint32_t hp2 = Ph >> 31, hn2 = Mh >> 31;
                Ph = (Ph << 1) | hp; Mh = (Mh << 1) | hn;
                Pv[w] = Mh | ~(Xv | Ph);
                Mv[w] = Ph & Xv;
                hp = hp2; hn = hn2;
            }
            msg = (int)(hp | (hn << 1));
            if (lg == toplane) {                            // M(len-1, y)
                score += (int)((tp >> bt) & 1u) - (int)((tn >> bt) & 1u);
                if (score < cutoff) {
                    if (!inrun) { inrun = 1; lo = y; mn = score; ey = y; }
                    else if (score <= mn) { mn = score; ey = y; }   // ties: the largest column (RC:562, scanned downward)
                } else if (inrun) {
                    if (nrun < jb.cap) runs[jb.roff + nrun] = make_int4(lo, y - 1, mn, ey);
                    ++nrun; inrun = 0;
                }
                if (inrun && y == L - 1) {
                    if (nrun < jb.cap) runs[jb.roff + nrun] = make_int4(lo, y, mn, ey);
                    ++nrun; inrun = 0;
                }
            }
        }
    }
    if (have && lg == toplane) counts[jid] = nrun;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct prc_ctx {
    int device = 0, T = 0;
    std::vector<char> templ;
    hipStream_t stream = nullptr;
    unsigned long long cells = 0;
    double kernel_ms = 0.0;
};

// the kernel takes a base's code from two bits of its character: anything else would silently alias one of the four
static inline bool rc_is_base(char ch)
{
    switch (ch) { case 'a': case 'c': case 'g': case 't': case 'A': case 'C': case 'G': case 'T': return true; default: return false; }
}

static int create(prc_ctx **out, const char *templ, int templ_len, int device)
{
    if (!out || (!templ && templ_len) || templ_len < 0) return PWR_ERR_ARG;
    for (int y = 0; y < templ_len; ++y) if (!rc_is_base(templ[y])) return PWR_ERR_INPUT;
    std::vector<char> copy(templ, templ + templ_len);                              // (before the context: nothing below throws)
    prc_ctx *c = new (std::nothrow) prc_ctx();
    if (!c) return PWR_ERR_NOMEM;
    c->device = device; c->T = templ_len;
    c->templ.swap(copy);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) { delete c; return PWR_ERR_DEVICE; }
    *out = c;
    return PWR_OK;
}

extern "C" int prc_create(prc_ctx **out, const char *templ, int templ_len, int device)
{
    return abi_guard([&] { return create(out, templ, templ_len, device); });
}

extern "C" void prc_destroy(prc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int prc_get_stats(prc_ctx *c, unsigned long long *cells, double *kernel_ms)
{
    if (!c) return PWR_ERR_ARG;
    if (cells) *cells = c->cells;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    return PWR_OK;
}

template <int WPL>
static void launch_rows(int wpl, bool both, dim3 grid, hipStream_t st, const uint32_t *planes, int nwords, int len, int cutoff, const char *bases,
                        const RcJob *jobs, const int *order, int njobs, int G, int4 *runs, int *counts)
{
    if (wpl == WPL) {
        if (both) hipLaunchKernelGGL((k_rc_rows<WPL, true>), grid, dim3(64), 0, st, planes, nwords, len, cutoff, bases, jobs, order, njobs, G, runs, counts);
        else hipLaunchKernelGGL((k_rc_rows<WPL, false>), grid, dim3(64), 0, st, planes, nwords, len, cutoff, bases, jobs, order, njobs, G, runs, counts);
        return;
    }
    if constexpr (WPL < RC_MAXWPL) launch_rows<WPL + 1>(wpl, both, grid, st, planes, nwords, len, cutoff, bases, jobs, order, njobs, G, runs, counts);
}

struct RcBufs {                     // freed on every way out
    char *bases = nullptr; uint32_t *planes = nullptr; RcJob *jobs = nullptr; int *order = nullptr; int4 *runs = nullptr; int *counts = nullptr;
    DevArena mem;                   // owns the six above
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~RcBufs()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// The rows of every (read, strand, queried piece) job, k = (j * ns + s) * nq + q with ns strands per read (1: forward only);
// on return run_off[k .. k+1) delimits job k's runs in `runs` (ascending columns of that orientation).
static int rc_rows(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap, double error_cutoff,
                   int ns, int *nq_out, int *len_out, std::vector<long long> &run_off, std::vector<int> &runs)
{
    if (!c || nreads < 0 || !off || (nreads && !bases)) return PWR_ERR_ARG;
    if (parts < 1) return PWR_ERR_ARG;                                             // RC:583 divides by it
    const int steps = c->T / parts, len = steps + overlap;                         // RC:583-585
    if (len < 0) return PWR_ERR_ARG;                                               // (the reference indexes Matrix[len - 1] < -1)
    const int cutoff = (int)((double)len * error_cutoff);
    const int nq = parts > 1 ? 2 : 1;                                              // RC:600: Occurrence for piece 0 and piece parts-1
    *nq_out = nq; *len_out = len;
    for (int j = 0; j < nreads; ++j) {
        const long long l = off[j + 1] - off[j];
        if (l < 0 || l > 0x7fffffff) return l < 0 ? PWR_ERR_ARG : PWR_ERR_RANGE;
    }
    const long long b0 = nreads ? off[0] : 0, nb = nreads ? off[nreads] - off[0] : 0;
    for (long long i = 0; i < nb; ++i) if (!rc_is_base(bases[b0 + i])) return PWR_ERR_INPUT;
    const long long njobs = (long long)nreads * ns * nq;
    run_off.assign((size_t)njobs + 1, 0);
    runs.clear();
    for (int j = 0; j < nreads; ++j) c->cells += (unsigned long long)(off[j + 1] - off[j]) * (unsigned long long)len * nq * ns;
    // len = 0: the last row is row -1, all 0, never below a cutoff of 0 (RC:534); a cutoff <= 0 is never undercut either
    if (len == 0 || cutoff <= 0 || njobs == 0) return PWR_OK;
    if (len > PRC_MAX_PART) return PWR_ERR_RANGE;
    if (njobs > 0x7fffffff) return PWR_ERR_RANGE;
    const int nwords = (len + 31) / 32;
    const int wpl = std::max(1, (nwords + 63) / 64);
    int G = 1;
    while (G * wpl < nwords) G *= 2;
    // piece planes (RC:601: &Template[i * steps], len bytes; past the template's end a byte that matches no base)
    std::vector<uint32_t> planes((size_t)nq * 3 * nwords, 0u);
    for (int q = 0; q < nq; ++q) {
        const long long start = (long long)(q == 0 ? 0 : parts - 1) * steps;
        uint32_t *pl = planes.data() + (size_t)q * 3 * nwords;
        for (int x = 0; x < len; ++x) {
            if (start + x >= c->T) continue;
            const int code = (c->templ[start + x] >> 1) & 3;
            if (code & 1) pl[x >> 5] |= 1u << (x & 31);
            if (code & 2) pl[nwords + (x >> 5)] |= 1u << (x & 31);
            pl[2 * nwords + (x >> 5)] |= 1u << (x & 31);
        }
    }
    std::vector<RcJob> hj((size_t)njobs);
    std::vector<int> order;
    order.reserve((size_t)njobs);
    long long roff = 0;
    for (int j = 0; j < nreads; ++j)
        for (int sq = 0; sq < ns * nq; ++sq) {
            const int k = j * ns * nq + sq;
            RcJob &jb = hj[(size_t)k];
            jb.boff = off[j] - b0; jb.L = (int)(off[j + 1] - off[j]); jb.pat = sq % nq; jb.cap = PRC_RUN_CAP; jb.strand = sq / nq;
            jb.roff = roff; roff += jb.cap;
            if (jb.L > 0) order.push_back(k);
        }
    // the longest reads first: neighbours in a wave run about as long, and the waves that run longest start first
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hj[a].L > hj[b].L; });
    std::vector<int> counts((size_t)njobs, 0);
    if (order.empty()) return PWR_OK;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    RcBufs d;
    HIPC(hipEventCreate(&d.e0)); HIPC(hipEventCreate(&d.e1));
    d.bases = d.mem.get<char>(nb); d.planes = d.mem.get<uint32_t>(planes.size()); d.jobs = d.mem.get<RcJob>(hj.size());
    d.order = d.mem.get<int>(order.size()); d.runs = d.mem.get<int4>(roff); d.counts = d.mem.get<int>(hj.size());
    if (!d.bases || !d.planes || !d.jobs || !d.order || !d.runs || !d.counts) return PWR_ERR_NOMEM;
    if (nb) HIPC(hipMemcpyAsync(d.bases, bases + b0, nb, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(d.planes, planes.data(), planes.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(d.jobs, hj.data(), sizeof(RcJob) * hj.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(d.order, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(d.counts, 0, sizeof(int) * hj.size(), c->stream));
    const int per = 64 / G;
    float ms = 0;
    HIPC(hipEventRecord(d.e0, c->stream));
    launch_rows<1>(wpl, ns == 2, dim3((unsigned)((order.size() + per - 1) / per)), c->stream, d.planes, nwords, len, cutoff, d.bases, d.jobs,
                   d.order, (int)order.size(), G, d.runs, d.counts);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(d.e1, c->stream));
    std::vector<int4> hr((size_t)roff);
    HIPC(hipMemcpyAsync(counts.data(), d.counts, sizeof(int) * hj.size(), hipMemcpyDeviceToHost, c->stream));
    if (roff) HIPC(hipMemcpyAsync(hr.data(), d.runs, sizeof(int4) * roff, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (hipEventElapsedTime(&ms, d.e0, d.e1) == hipSuccess) c->kernel_ms += ms;
    // overflow: every job with more runs than room goes again, with exactly the room it reported
    std::vector<int> again;
    long long roff2 = 0;
    for (int k : order)
        if (counts[k] > hj[k].cap) { again.push_back(k); hj[k].cap = counts[k]; hj[k].roff = roff2; roff2 += counts[k]; }
    std::vector<int4> hr2((size_t)roff2);
    if (!again.empty()) {
        int4 *runs2 = nullptr;                                                     // (freed as soon as its runs are on the host)
        if (hipMalloc(&runs2, sizeof(int4) * roff2) != hipSuccess) return PWR_ERR_NOMEM;
        std::vector<int> counts2((size_t)njobs, 0);
        int rc = PWR_OK;
        if (hipMemcpyAsync(d.jobs, hj.data(), sizeof(RcJob) * hj.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d.order, again.data(), sizeof(int) * again.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipEventRecord(d.e0, c->stream) != hipSuccess) rc = PWR_ERR_DEVICE;
        if (rc == PWR_OK) {
            launch_rows<1>(wpl, ns == 2, dim3((unsigned)((again.size() + per - 1) / per)), c->stream, d.planes, nwords, len, cutoff, d.bases,
                           d.jobs, d.order, (int)again.size(), G, runs2, d.counts);
            if (hipGetLastError() != hipSuccess || hipEventRecord(d.e1, c->stream) != hipSuccess ||
                hipMemcpyAsync(counts2.data(), d.counts, sizeof(int) * hj.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipMemcpyAsync(hr2.data(), runs2, sizeof(int4) * roff2, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess) rc = PWR_ERR_DEVICE;
        }
        (void)hipFree(runs2);
        if (rc != PWR_OK) return rc;
        if (hipEventElapsedTime(&ms, d.e0, d.e1) == hipSuccess) c->kernel_ms += ms;
        for (int k : again) if (counts2[k] != hj[k].cap) return PWR_ERR_INTERNAL;  // the same job counts the same runs
    }
    std::vector<char> redo((size_t)njobs, 0);
    for (int k : again) redo[k] = 1;
    for (long long k = 0; k < njobs; ++k) run_off[k + 1] = run_off[k] + counts[k];
    runs.resize((size_t)run_off[njobs] * 4);
    for (long long k = 0; k < njobs; ++k) {
        const int4 *src = redo[k] ? hr2.data() + hj[k].roff : hr.data() + hj[k].roff;
        for (int r = 0; r < counts[k]; ++r) {
            int *dst = runs.data() + (run_off[k] + r) * 4;
            dst[0] = src[r].x; dst[1] = src[r].y; dst[2] = src[r].z; dst[3] = src[r].w;
        }
    }
    return PWR_OK;
}

static int occurrences(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap, double error_cutoff,
                       int ns, long long *pos_off, int **pos)
{
    if (!pos_off || !pos) return PWR_ERR_ARG;
    int nq = 0, len = 0;
    std::vector<long long> run_off;
    std::vector<int> runs;
    const int rc = rc_rows(c, nreads, bases, off, parts, overlap, error_cutoff, ns, &nq, &len, run_off, runs);
    if (rc != PWR_OK) return rc;
    const long long njobs = (long long)nreads * ns * nq;
    int *p = (int *)malloc(sizeof(int) * (size_t)std::max<long long>(run_off[njobs], 1));
    if (!p) return PWR_ERR_NOMEM;
    pos_off[0] = 0;
    for (long long k = 0; k < njobs; ++k) {
        const int n = prc_scan_runs(runs.data() + run_off[k] * 4, (int)(run_off[k + 1] - run_off[k]), len, p + pos_off[k]);
        pos_off[k + 1] = pos_off[k] + n;
    }
    *pos = p;
    return PWR_OK;
}

extern "C" int prc_occurrences(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap,
                               double error_cutoff, long long *pos_off, int **pos)
{
    return abi_guard([&] { return occurrences(c, nreads, bases, off, parts, overlap, error_cutoff, 1, pos_off, pos); });
}

extern "C" int prc_occurrences_strands(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap,
                                       double error_cutoff, long long *pos_off, int **pos)
{
    return abi_guard([&] { return occurrences(c, nreads, bases, off, parts, overlap, error_cutoff, 2, pos_off, pos); });
}

// nfwd == nullptr: prc_cut.  Otherwise FullAnalysis once per orientation, the two lists merged into the read's coordinates.
static int cut(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap, double error_cutoff, int *ncut,
               int **cuts, int *nfwd, int *nrev)
{
    if (!ncut || !cuts) return PWR_ERR_ARG;
    const int ns = nfwd ? 2 : 1;
    int nq = 0, len = 0;
    std::vector<long long> run_off;
    std::vector<int> runs;
    const int rc = rc_rows(c, nreads, bases, off, parts, overlap, error_cutoff, ns, &nq, &len, run_off, runs);
    if (rc != PWR_OK) return rc;
    const long long njobs = (long long)nreads * ns * nq;
    // positions <= runs per job; cut points <= 3 * n0 + 2 * nL + 1 per read and orientation
    std::vector<int> pos((size_t)std::max<long long>(run_off[njobs], 1));
    std::vector<long long> cut_off((size_t)nreads + 1, 0);
    long long widest = 1;
    for (int j = 0; j < nreads; ++j) {
        const long long room = 3 * (run_off[(size_t)(j + 1) * ns * nq] - run_off[(size_t)j * ns * nq]) + ns;
        cut_off[j + 1] = cut_off[j] + room;
        widest = std::max(widest, room);
    }
    std::vector<int> both((size_t)(ns == 2 ? 2 * widest : 0));                          // one read's two lists before the merge
    int *out = (int *)malloc(sizeof(int) * (size_t)std::max<long long>(cut_off[nreads], 1));
    if (!out) return PWR_ERR_NOMEM;
    long long w = 0;
    for (int j = 0; j < nreads; ++j) {
        const int readlen = (int)(off[j + 1] - off[j]);
        int n_of[2] = {0, 0};
        for (int s = 0; s < ns; ++s) {
            const long long k0 = ((long long)j * ns + s) * nq;
            int *p0 = pos.data() + run_off[k0];
            const int n0 = prc_scan_runs(runs.data() + run_off[k0] * 4, (int)(run_off[k0 + 1] - run_off[k0]), len, p0);
            int *pL = p0, nL = n0;
            if (nq == 2) {
                pL = pos.data() + run_off[k0 + 1];
                nL = prc_scan_runs(runs.data() + run_off[k0 + 1] * 4, (int)(run_off[k0 + 2] - run_off[k0 + 1]), len, pL);
            }
            int *dst = ns == 2 ? both.data() + (size_t)s * widest : out + w;
            n_of[s] = prc_select_cuts(parts, len, c->T, readlen, p0, n0, pL, nL, dst);
            if (n_of[s] < 0) { free(out); return n_of[s]; }
        }
        int n = n_of[0];
        if (ns == 2) {
            n = prc_merge_cuts(readlen, n_of[0], both.data(), n_of[1], both.data() + widest, out + w);
            if (n < 0) { free(out); return n; }
            nfwd[j] = n_of[0]; nrev[j] = n_of[1];
        }
        ncut[j] = n;
        w += n;
    }
    *cuts = out;
    return PWR_OK;
}

extern "C" int prc_cut(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap, double error_cutoff,
                       int *ncut, int **cuts)
{
    return abi_guard([&] { return cut(c, nreads, bases, off, parts, overlap, error_cutoff, ncut, cuts, nullptr, nullptr); });
}

extern "C" int prc_cut_strands(prc_ctx *c, int nreads, const char *bases, const long long *off, int parts, int overlap,
                               double error_cutoff, int *ncut, int **cuts, int *nfwd, int *nrev)
{
    return abi_guard([&] {
        if (!nfwd || !nrev) return (int)PWR_ERR_ARG;
        return cut(c, nreads, bases, off, parts, overlap, error_cutoff, ncut, cuts, nfwd, nrev);
    });
}
