// pgr_win_device.hip -- MI355X (gfx950): RepeatResolver's window reader on a device-resident MSA, and the resolution of
// several windows in one call, behind include/pgr.h (pgr_msa_*).
//
// Reference: PhilippBongartz/RepeatResolver, RepeatResolver.c ("RR:"), Einlesen (RR:293-429): a row is kept when neither end
// column of the window is ' ' (RR:330); bit j of every set is the j-th kept row (RR:332, RR:410); per column five group sets,
// the coverage set and Coverage.
//   k_win_kept   a thread per row: the two end columns of the window.
//   k_win_bits   a thread per (column, 64-row word) as k_mc_bits of pmc_device.hip: the list of kept rows takes the place of
//                its `inv`; the threads of a wave read neighbouring columns of one row; the sets are written word-major
//                (G[w][column * 5 + symbol], LC[w][column]) as k_gr_cliques and k_gr_votes read them.  Group sizes and
//                Coverage are sums of popcounts: integers, so the order of the atomics does not matter.
// The list of kept rows is made on the host from the downloaded flags (at most PGR_MAX_ROWS bytes).
// Every index into the text is 64-bit: rows * width exceeds 2^31 at the size of a real data set.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PWR_STAGE "pgr"
#include "base_code.h"
#include "dev_util.h"
#include "pgr.h"
#include "pgr_internal.h"

static double g_rs_ms[7] = {0, 0, 0, 0, 0, 0, 0};

__global__ __launch_bounds__(256) void k_win_kept(int rows, long long width, int von, int bis, const unsigned char *__restrict__ text,
                                                  unsigned char *__restrict__ flag)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const unsigned char *line = text + (long long)r * width;
    flag[r] = line[von] != ' ' && line[bis] != ' ';                    // RR:330
}

// grid (columns of the window / 256, sc); list[nk] = the kept rows, ascending
__global__ __launch_bounds__(256) void k_win_bits(int nk, int W, long long width, int von, const unsigned char *__restrict__ text,
                                                  const int *__restrict__ list, unsigned long long *__restrict__ G,
                                                  unsigned long long *__restrict__ LC, int *__restrict__ gsize, int *__restrict__ cover)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    if (c >= W) return;
    unsigned long long g[5] = {0, 0, 0, 0, 0};
    const int n = min(64, nk - w * 64);                                // (the last word may hold no row at all: sc = nk / 64 + 1)
    for (int r = 0; r < n; ++r) {
        const int k = base_code(text[(long long)list[w * 64 + r] * width + von + c]);
#pragma unroll
        for (int q = 0; q < 5; ++q) g[q] |= (unsigned long long)(k == q) << r;
    }
    unsigned long long lc = 0;
    const size_t V = (size_t)W * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        G[(size_t)w * V + (size_t)c * 5 + k] = g[k];
        lc |= g[k];
        if (g[k]) atomicAdd(&gsize[c * 5 + k], __popcll(g[k]));
    }
    LC[(size_t)w * W + c] = lc;
    if (lc) atomicAdd(&cover[c], __popcll(lc));
}

// a window's sets on the device and what the host knows of it
struct DevWindow {
    int rows = 0, kept_rows = 0, von = 0, bis = 0, width = 0, sc = 0;
    unsigned long long *G = nullptr, *LC = nullptr;
    int *gsize = nullptr, *cover = nullptr, *list = nullptr;
    unsigned char *flag = nullptr;
    std::vector<unsigned char> kept;
    DevArena mem;                                                      // owns the pointers above
};

// Einlesen on the device: the argument checks and their order are pgr_read_window's
static int read_on_device(const pgr_msa *h, int von, int bis, DevWindow &d)
{
    const int rows = h->rows, width = h->width;
    if (von == -1 && bis == -1) { von = 0; bis = PGR_MAX_COLUMNS; }                // RR:3948-3952
    if (bis > width - 1) bis = width - 1;                                          // RR:328
    if (von < 0 || von > bis) return PWR_ERR_ARG;
    const int W = bis + 1 - von;                                                   // RR:374
    d.rows = rows; d.von = von; d.bis = bis; d.width = W;
    if (hipSetDevice(h->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (!(d.flag = d.mem.get<unsigned char>(rows))) return PWR_ERR_NOMEM;
    hipLaunchKernelGGL(k_win_kept, dim3((rows + 255) / 256), dim3(256), 0, 0, rows, (long long)width, von, bis, h->text, d.flag);
    HIPC(hipGetLastError());
    d.kept.resize((size_t)rows);
    HIPC(hipMemcpy(d.kept.data(), d.flag, (size_t)rows, hipMemcpyDeviceToHost));
    std::vector<int> list;
    for (int r = 0; r < rows; ++r) if (d.kept[r]) list.push_back(r);
    const int nk = (int)list.size(), sc = nk / 64 + 1;                             // RR:375
    d.kept_rows = nk; d.sc = sc;
    const size_t V = (size_t)W * 5;
    d.G = d.mem.get<unsigned long long>(V * sc); d.LC = d.mem.get<unsigned long long>((size_t)W * sc);
    d.gsize = d.mem.get<int>(V); d.cover = d.mem.get<int>(W); d.list = d.mem.put(list.data(), nk);
    if (!d.G || !d.LC || !d.gsize || !d.cover || !d.list) return d.mem.err;
    HIPC(hipMemset(d.gsize, 0, V * 4));
    HIPC(hipMemset(d.cover, 0, (size_t)W * 4));
    hipLaunchKernelGGL(k_win_bits, dim3((W + 255) / 256, sc), dim3(256), 0, 0, nk, W, (long long)width, von, h->text, d.list, d.G, d.LC, d.gsize,
                       d.cover);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    return PWR_OK;
}

// the host's pgr_window of a device window: one download, the sets turned set-major as Einlesen leaves them
static int download(const DevWindow &d, pgr_window *win)
{
    const int W = d.width, sc = d.sc;
    const size_t V = (size_t)W * 5;
    win->rows = d.rows; win->kept_rows = d.kept_rows; win->von = d.von; win->bis = d.bis; win->width = W; win->sc = sc;
    win->kept = (unsigned char *)malloc((size_t)d.rows);
    win->groups = (unsigned long long *)calloc(V * sc, 8);
    win->local_coverage = (unsigned long long *)calloc((size_t)W * sc, 8);
    win->coverage = (int *)calloc((size_t)W, sizeof(int));
    if (!win->kept || !win->groups || !win->local_coverage || !win->coverage) return PWR_ERR_NOMEM;
    memcpy(win->kept, d.kept.data(), (size_t)d.rows);
    HIPC(hipMemcpy(win->coverage, d.cover, (size_t)W * 4, hipMemcpyDeviceToHost));
    if (sc == 1) {                                                                 // one word: both layouts are the same
        HIPC(hipMemcpy(win->groups, d.G, V * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(win->local_coverage, d.LC, (size_t)W * 8, hipMemcpyDeviceToHost));
        return PWR_OK;
    }
    std::vector<unsigned long long> t(V * sc);
    HIPC(hipMemcpy(t.data(), d.G, V * sc * 8, hipMemcpyDeviceToHost));
    pgr_word_major(t.data(), (int)V, nullptr, (size_t)sc, win->groups);                // (the way back: the extents exchanged)
    HIPC(hipMemcpy(t.data(), d.LC, (size_t)W * sc * 8, hipMemcpyDeviceToHost));
    pgr_word_major(t.data(), W, nullptr, (size_t)sc, win->local_coverage);
    return PWR_OK;
}

extern "C" int pgr_msa_open(int rows, int width, const unsigned char *text, int device, pgr_msa **h)
{
    if (!h) return PWR_ERR_ARG;
    *h = nullptr;
    if (rows <= 0 || width <= 0 || !text) return PWR_ERR_ARG;
    if (rows > PGR_MAX_ROWS || width > PGR_MAX_COLUMNS - 3) return PWR_ERR_RANGE;  // RR:291, RR:322
    const double t0 = now_ms();
    if (hipSetDevice(device) != hipSuccess) return PWR_ERR_DEVICE;
    pgr_msa *m = (pgr_msa *)calloc(1, sizeof *m);
    if (!m) return PWR_ERR_NOMEM;
    m->rows = rows; m->width = width; m->device = device;
    const size_t bytes = (size_t)rows * (size_t)width;
    // (bytes + 3: a whole number of 32-bit words, k_cs_counts of pgr_cons_device.hip reads the text as words)
    if (hipMalloc(&m->text, bytes + 3) != hipSuccess) { (void)hipGetLastError(); free(m); return PWR_ERR_NOMEM; }
    if (hipMemcpy(m->text, text, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(m->text); free(m); return PWR_ERR_DEVICE; }
    g_rs_ms[0] = now_ms() - t0;
    *h = m;
    return PWR_OK;
}

extern "C" void pgr_msa_close(pgr_msa *h)
{
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) (void)hipFree(h->text);
    free(h);
}

extern "C" int pgr_msa_window(pgr_msa *h, int von, int bis, pgr_window *win)
{
    if (!win) return PWR_ERR_ARG;
    memset(win, 0, sizeof *win);
    if (!h) return PWR_ERR_ARG;
    const int rc = abi_guard([&] {
        DevWindow d;
        const int rd = read_on_device(h, von, bis, d);
        return rd ? rd : download(d, win);
    });
    if (rc) pgr_window_free(win);
    return rc;
}

extern "C" void pgr_resolution_free(pgr_resolution *o)
{
    if (!o) return;
    for (int p = 0; o->windows && p < o->nwindows; ++p) {
        free(o->windows[p].dropoff_labels); free(o->windows[p].reldrop_labels); free(o->windows[p].kmeans_labels);
    }
    free(o->windows);
    memset(o, 0, sizeof *o);
}

extern "C" int pgr_last_resolve_timing(double *ms7)
{
    if (!ms7) return PWR_ERR_ARG;
    for (int i = 0; i < 7; ++i) ms7[i] = g_rs_ms[i];
    return PWR_OK;
}

namespace {
struct StageGuard {
    pgr_window win;
    pgr_result res;
    pgr_subdivision sd;
    pgr_kmeans km;
    StageGuard() { memset(&win, 0, sizeof win); memset(&res, 0, sizeof res); memset(&sd, 0, sizeof sd); memset(&km, 0, sizeof km); }
    ~StageGuard() { pgr_kmeans_free(&km); pgr_subdivision_free(&sd); pgr_free(&res); pgr_window_free(&win); }
};
}

static int resolve_window(pgr_msa *h, const double *maxcorrs_full, int von, int bis, int mincov, double cutoff, pgr_resolved_window *o)
{
    const size_t nb = sizeof(int) * (size_t)h->rows;
    StageGuard s;
    DevWindow d;
    double t = now_ms(), u;
    int rc = read_on_device(h, von, bis, d);
    if (rc) return rc;
    u = now_ms(); g_rs_ms[2] += u - t; t = u;
    if ((rc = download(d, &s.win))) return rc;
    u = now_ms(); g_rs_ms[3] += u - t; t = u;
    pgr_device_sets sets = {d.rows, d.kept_rows, d.von, d.bis, d.width, d.sc, d.G, d.LC, d.gsize};
    if ((rc = pgr_refine_sets(&sets, s.win.kept, s.win.coverage, maxcorrs_full, h->width, mincov, cutoff, h->device, &s.res, nullptr))) return rc;
    u = now_ms(); g_rs_ms[4] += u - t; t = u;
    if ((rc = pgr_subdivide(&s.win, &s.res, mincov, h->device, &s.sd))) return rc;
    u = now_ms(); g_rs_ms[5] += u - t; t = u;
    if ((rc = pgr_kmeans_subdivide(&s.win, &s.res, s.sd.reldrop_labels, mincov, h->device, &s.km))) return rc;
    g_rs_ms[6] += now_ms() - t;
    o->von = von; o->bis = bis; o->kept_rows = d.kept_rows; o->cutoff = s.res.cutoff;
    o->dropoff_parts = s.sd.dropoff_parts; o->reldrop_parts = s.sd.reldrop_parts; o->kmeans_parts = s.km.parts;
    o->dropoff_labels = (int *)malloc(nb); o->reldrop_labels = (int *)malloc(nb); o->kmeans_labels = (int *)malloc(nb);
    if (!o->dropoff_labels || !o->reldrop_labels || !o->kmeans_labels) return PWR_ERR_NOMEM;
    memcpy(o->dropoff_labels, s.sd.dropoff_labels, nb); memcpy(o->reldrop_labels, s.sd.reldrop_labels, nb); memcpy(o->kmeans_labels, s.km.labels, nb);
    return PWR_OK;
}

extern "C" int pgr_msa_resolve(pgr_msa *h, const double *maxcorrs_full, int nsites, const int *sites, int mincov, double cutoff,
                               pgr_resolution *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!h || !maxcorrs_full || !sites || nsites < 2 || mincov < 0 || !(cutoff <= 100.0)) return PWR_ERR_ARG;
    for (int p = 0; p < nsites; ++p)
        if (sites[p] < 0 || (p > 0 && sites[p] <= sites[p - 1])) return PWR_ERR_ARG;
    const double t0 = now_ms();
    for (int i = 1; i < 7; ++i) g_rs_ms[i] = 0;
    out->rows = h->rows; out->nwindows = nsites - 1;
    out->windows = (pgr_resolved_window *)calloc((size_t)(nsites - 1), sizeof(pgr_resolved_window));
    if (!out->windows) { pgr_resolution_free(out); return PWR_ERR_NOMEM; }
    for (int p = 0; p + 1 < nsites; ++p) {
        const int rc = abi_guard([&] { return resolve_window(h, maxcorrs_full, sites[p], sites[p + 1], mincov, cutoff, out->windows + p); });
        if (rc) { pgr_resolution_free(out); return rc; }
    }
    g_rs_ms[1] = now_ms() - t0;
    return PWR_OK;
}
