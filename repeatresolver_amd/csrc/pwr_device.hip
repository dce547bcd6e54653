// pwr_device.hip -- MI355X (gfx950) implementation of the PW_ReAligner hot path behind include/pwr.h.
//
// Reference: PhilippBongartz/RepeatResolver, PW_ReAligner.c ("PW:").  Nothing here is translated
// from it; the reference is a single-threaded walk over a linked list of columns with a 64-bit
// L x 2000 score matrix.  This file keeps the MSA resident in HBM as
//   * per row:    its base sequence (static) and, per base, the id ("slot") of the column holding it,
//   * per column: the six tallies w_con[0..5] of PW:41-47 plus the number of rows that END in it,
//   * the column order (ordinal -> slot) and its inverse (slot -> ordinal),
// and realigns a row with four kernels: gather (TheWay + Downdater, PW:647-705/1172-1220, into
// job-private DP inputs), fill (PW:1493-1513), trace (PW:1334-1454) and commit (Column_Updater /
// Column_Adder / W_Con, PW:1222-1332, PW:706-763).  See DESIGN.md for the derivations.
//
// Symbols 0..3 = A,C,G,T, 4 = '-', 5 = ' '.  w[b] = #rows non-blank and != b in the column.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "pwr.h"

#define PWR_INF 0x40000000u        // any value >= this is "unreachable"; finite scores stay below (range check)
#define PWR_BIG 0x7fffffff

// ---------------------------------------------------------------------------------------------
// device-side data
// ---------------------------------------------------------------------------------------------
struct Hdr {                       // lives in device memory, one per context
    int W;                         // current width (Breite, PW:87)
    int nslots;                    // column slots ever handed out
    int nfree;                     // entries on the free list (the Reservoir of PW:51)
    int cur;                       // which of the two order buffers is current
    int status;                    // sticky error (PWR_ERR_*), 0 = fine
    int stop;                      // batch mode: set when a speculative job failed validation
    int ncommitted;                // batch mode: jobs committed in the current batch
    int version;                   // bumped by every commit that changes the state: names the state a job's inputs were gathered from
    unsigned long long cells_computed;
    unsigned long long cells_reference;
    unsigned long long rows_changed;   // commits that changed at least one column
    unsigned long long fail_reason[4]; // why speculative jobs were rejected: 0 ends/length, 1 left clamp, 2 right clamp, 3 newer column
    unsigned long long batches, rows_committed, rows_recomputed;   // speculative batches with work; realignments committed / thrown away
    unsigned long long rows_wide;      // committed realignments that were filled by k_fill64
    unsigned long long stalls;         // k_fill_v3 jobs given up because a wave waited too long for its neighbour
    unsigned long long rows_ahead;     // commits that went ahead of a stale row of the same batch
    unsigned long long seg_jobs, segs, seg_fails;   // segmented fills: jobs cut into more than one segment, their segments, jobs whose check failed
    int agree, pad0;               // the two order buffers hold the same ordinals for the columns [0, agree)
    // the k loop (PW:1695) is sequenced on the device: a batch realigns the rows rowids[next_row ...], its commit kernel moves
    // next_row on and sizes the next batch, so the host enqueues batches without waiting for their outcome
    int next_row, row_end;         // rows [next_row, row_end) of the current slab are still to do
    int nb;                        // rows the next batch gathers (the first is certain to commit, the others are speculative)
    int need_grow;                 // a commit found the column arrays too small: nothing happens until the host has regrown them
    int window;
    int fallback;                  // > 0: this many batches are filled by k_fill_v2 (one work-group per job, no waiting across work-groups)
    float ema;                     // running mean of rows committed per batch
    int speclen;                   // a speculative row may be this many percent longer than the batch's first row
    unsigned long long ahead;      // bit b: row next_row + b was committed ahead of an earlier, stale row it commutes with (its band
                                   // interval is disjoint from that row's), so the batches to come leave it out
    int noseg_row;                 // this row's segmented fill failed its check (-1: none) ...
    int noseg_level;               // ... once: its next fill warms up twice as long; twice: it runs in one piece
    unsigned seq;                  // host copy only: which batch this copy of the header belongs to (written last)
    int need64;                    // > 0: a job needed the 64-bit fill lately; the host launches k_fill64 with the batches while this counts down
    // How long a segment warms up is steered by how often the check fails (k_commit_chain): every segmented fill that passes
    // takes warm_step columns off, every one that fails puts warm_up (ten times as many) back on -- the length settles where
    // about one fill in ten is repeated, which is where a longer warm-up for all costs as much as the repeats it saves
    // (measured).
    // Results never depend on it.  warm_step 0: fixed length (JobBufs::warm_cols).
    int warm_cur, warm_lo, warm_hi, warm_step, warm_up;   // (warm_up: columns a failure puts back on)
    // Rows picked AHEAD of rows that are not in their batch (k_commit_finish): bit b of jumpmask = row next_row + b is one; the
    // structural events (columns opened / emptied) committed so far and their running mean per commit: a row jumps only while
    // 64 commits' worth of events stay far below the gap it keeps, and every row that was jumped over checks at its gather that
    // the gap has held (k_gather_a) -- exactness is checked, not assumed.
    unsigned long long jumpmask;
    unsigned long long events_total, rows_jumped;
    float evrate; int pad1;
    unsigned long long hard_marked, hard_fills, hard_refail;   // "hard_rows": rows marked; fills of marked rows planned like any other; those of them that failed
    unsigned long long dbg[32];    // phase timers of the traceback (10 ns ticks), only written by builds with -DPWR_DIAG
};

struct Tally {                     // 32 B per column slot
    uint32_t w[6];                 // PW:46 w_con
    uint32_t endcnt;               // rows whose last base sits in this column
    uint32_t pad;
};

struct JobMeta {                   // 96 B
    int k, L, lo, hi, W, entry, ok, nnew;
    unsigned maxS;
    int ver;                       // hdr->version when the job's inputs were gathered
    unsigned long long cells;
    int slot_lo, slot_hi;          // column slots at both ends of the gathered interval
    unsigned clk, rclk;            // fill kernel duration in shader clocks / 100 MHz ticks (diagnostic)
    int rounds;                    // lock-step rounds the fill needed (diagnostic)
    int abort;                     // k_fill_v3: a wave gave up waiting; its siblings leave too
    int active;                    // 0: the job slot is unused in this batch (everything else is left from the last use)
    int wide;                      // 1: the scores may not fit 32 bits: k_fill64 fills this job, the wave pipeline skips it
    int off, hard;                 // the job's row is rowids[next_row + off]; hard: bit 0 = the row is marked (DState::hard), bit 1 = its fill warmed up the long way for that
    int changed, level;            // (level: how often the row's check had failed when this fill was planned)  changed 0: the traceback left every base where it was (k_trace_blk): the commit has nothing to do
    int nseg, segfail;             // segments the fill was cut into (k_fill_v3); 1: a segment's warm-up had not converged, the job is repeated in one piece
};

struct DState {
    Hdr *hdr;
    int T, B, H, Lmax;
    int colcap, slotcap;
    const long long *rowoff;
    const int *rowlen;
    const uint8_t *seq;
    int *pos;
    Tally *tally;
    int *order0, *order1;
    int *rank;
    int *freelist;
    // rows that came in with blanks BETWEEN their bases (never written by the pipeline, but the reference reads them,
    // PW:165-222): such a row is a chain of segments base..base separated by blank runs until its first realignment makes
    // it one piece (PW:1362-1443).  brkx[brkoff[k] .. + nbrk[k]) = indices of the bases after which a blank run follows.
    const long long *brkoff;
    const int *brkx;
    int *nbrk;                     // [T] cleared by the row's first commit
    int *hard;                     // [T] "hard_rows": > 0 = a segmented fill of this row failed its check lately (k_commit_finish); such a row warms up the long way at once
    int *inscnt;                   // scratch [colcap], kept all-zero between commits
    int *newidx;                   // scratch [colcap]
    // The rows of the NEXT batch, picked by the batch before it (k_commit_finish): [0] 1 = the list is valid (0: the next rows in
    // order), [1 + j] offset of job j's row from Hdr::next_row, [1 + PLAN_MAX + j] for a row picked AHEAD of rows that are not
    // in the batch: its distance in columns to the nearest of their intervals (INT_MAX for the rows taken in order).
    int *bplan;
};
#define PLAN_MAX 16                 // jobs a planned batch may have ("window" beyond that: rows in order)
#define JR_BASE (1 + 2 * PLAN_MAX)  // behind the plan: one record per row that jumped, at (row index & 63): {events_total at its commit,
                                    // columns of its interval left of its first base, right of its last base (own new columns included), -}
#define BPLAN_WORDS (JR_BASE + 64 * 4)
#define PLAN_CAND 128               // rows k_commit_finish looks up beside its header work (the row pointer moves by at most 64)
#define PLAN_EVRATE_MAX 12.0f       // rows jump only while a commit opens / empties fewer columns than this on average
#define PLAN_SLACK 2048               // a row is picked ahead only if its interval keeps this many columns (+ 2) from every row it jumps

// A DP is filled in SEGMENTS that run side by side (k_fill_v3): segment s owns the DP rows [xown, xe) and starts WARM rows
// earlier, at xb, from a start of its own (one cell: the column of the base before row xb; or the free start of PW:265, as if
// row xb were the row's first base -- see k_fill_v3).  The fill is a min-plus recurrence
// whose row vectors forget where they started: after the band has moved past the columns of the start row they are PARALLEL to
// the true ones (equal up to one additive constant over the whole band), and from there on every comparison the traceback
// record is made of comes out the same.  Whether the warm-up got there is CHECKED, not assumed (k_seg_check compares the
// scores of row xown - 1 as the segment has them with those its predecessor ends on); a job that fails is filled again in
// one piece.  (Rank convergence of tropical DP; measured for this band: scripts/dev/rank_convergence.py.)
#define SEG_MAX 256
struct SegDesc {
    int job, s;                    // job slot, index of the segment within the job
    int xb, xown, xe;              // warm-up from xb, own rows [xown, xe)
    int fin, active;               // the job's last segment (holds the DP's last row); 0: slot unused in this launch
    int grow0;                     // row of the job's mailbox area (gmb) that holds the segment's row xb
    unsigned long long cells;      // DP cells of the rows [xb, xe)
};
struct GatherPart;
struct CommitJob {                  // what k_commit_scan found out about a job (reset by the job's gather)
    int nchg, nev, ndel, first;     // columns whose symbol changes, structural events, columns emptied, first ordinal with an event
    int u0, u1;                     // the columns the row covers before or after: every change lies in [u0, u1], every event in [u0 - 1, u1]
    int scanned, pad;
};
struct JobBufs {
    GatherPart *gpart;             // [njobs][GATHER_G] partial results of the gather's shares
    unsigned gather_tag;           // launch counter of the gather (tags the partial results)
    JobMeta *meta;
    int *way;                      // [njobs][Lmax]   ordinal of every base (PW:31 Way)
    int4 *rec2;                    // [njobs][2*colcap] the same pre-combined for k_fill_v2: {S0-G,S1-G,S2-G,S3-G},{up-G,G,INF-G,0}
    uint8_t *mark;                 // [njobs][colcap] old symbol marks (base+1 / 0)
    uint8_t *mark2;                // [njobs][colcap] new symbol marks
    uint32_t *dirs;                // [njobs][dirstride] traceback record, 2 bits per DP cell
    int *newcol;                   // [njobs][Lmax]   (ordinal << 1) | opened-a-new-column
    int *aux;                      // [njobs][Lmax]   slot of every base after the commit
    uint4 *desc;                   // [njobs][Lmax]   per DP row: {anf | base << 24, flags of waves 0-7, 8-15, 16-23} (4 bits per wave)
    int wpNW, wpMS;                // geometry of the wave pipeline the descriptors are made for
    unsigned *lastM;               // [njobs][NC]     scores of the last DP row (wave-pipeline fill)
    unsigned long long *gmb;       // [njobs][NW][gstride] k_fill_v3: {P_end, tag} per wave and DP row (segments side by side)
    SegDesc *seg;                  // [njobs][SEG_MAX] plan of the fill (plan_segments, with k_gather_c)
    unsigned *chk;                 // [njobs][SEG_MAX + 1][2][NC] scores of the row before segment s: [0] as s has them after its warm-up, [1] as s - 1 ends
    int seg_align;                 // own parts start at multiples of this (16, 32 or 64)
    int src_start;                 // 1: a warm-up starts from the column of the base before it alone (k_fill_v3), 0: from the free start
    int smax, seg_rows, warm_cols; // at most smax segments per job, of about seg_rows own rows, warmed up over warm_cols columns of band movement
    int seg_budget, seg_minrows;   // segments all jobs of a batch may have together (dealt by length), none with fewer own rows than seg_minrows
    int seg_balance;               // 1: the own parts are cut so that all segments of a job run about the same number of rows, warm-up included
    int plan_ahead;                // 1: the rows of a batch are picked by the batch before it: rows that commute with every row before them first
    int hard_rows, hard_up, hard_down;  // a row whose check fails warms up over hard_up more columns from then on, hard_down fewer after every commit (1; 2 = only counted)
    int plan_len;                       // > 0: a row is picked ahead only if it is at most this many percent longer than the batch's first row (0: any length)
    int plan_gate_rel;                  // 1: rows jump only while 64 commits' worth of events stay below half the gap they keep (0: test hook)
    int spec_inorder;                   // with plan_ahead: at most this many speculative rows in order per batch, beside the rows picked ahead
    int fail_stops;                     // 1: a job that failed its segment check ends its batch (test hook; 0: later rows that commute with it may still commit)
    int plan_slack, plan_evrate_x100;   // ... which keep more than this many columns from them; only while a commit opens / empties fewer columns than this / 100 on average
    const int *rowids;             // the slab's rows (the plan of a job looks at the lengths of the batch's other jobs)
    int gstride;                   // rows per wave of a job's mailbox area
    unsigned tagbase;              // launch epoch << 17: tags of this launch are tagbase | (row + 1)
    unsigned long long *gtr;       // [njobs][trk]    k_trace_par / k_trace_blk: hand-over words of the chunks
    int trk;                       // ... per job: max(TRK, Lmax / TB_C + 1)
    unsigned trace_tag;            // 14-bit launch tag of those words
    long long *g64;                // [njobs][colcap] k_fill64: 64-bit prefix sums of S(.,4)
    int force64;                   // test hook: every job takes the 64-bit fill
    int evcap;                     // commits with more structural events than this renumber by a pass over the width (test hook; <= EVCAP)
    int gate_v2;                   // k_fill_v2 launched behind k_fill_v3: it runs only while Hdr::fallback > 0
    int *chkdone;                  // [njobs] boundaries of the job's fill that k_seg_check has been through (reset by the gather)
    int check_in_trace, trace_ny;  // the check's work-groups ride in k_trace_blk's launch, behind its trace_ny rows of work-groups (one launch less per batch)
    int trace_prior;               // k_trace_blk takes the rows that keep their place a run at a time (`trace_prior`)
    int trace_blk;                 // this batch's traceback is k_trace_blk's (its chunk words carry the 'up' moves of every 64 rows)
    int v2_follows, f64_follows;   // this batch's launches include the stand-in k_fill_v2 / the 64-bit k_fill64 (the host adds them when the
                                   // header it last saw says they are wanted; a job that wanted one in a batch without it is repeated)
    int stall_test;                // test hook: job 0 of this k_fill_v3 launch pretends its neighbour never answers
    unsigned long long *diag;      // [njobs][32][4096] per-wave counters, switch events and a progress log of k_fill_v3 (only written when built with -DPWR_DIAG)
    int njobs_launched;
    int Lmax, colcap, NC;
    size_t dirstride;
    // One round split over the GPUs of a node (pwr_split_*): every rank holds the whole state and gathers every
    // job of a batch, but fills and traces only the jobs j with j % split_world == split_rank; the others' placements arrive
    // through the all-gather, and every rank commits all of them in row order.  split_world <= 1: everything is this rank's.
    int split_rank, split_world;
    // commit (k_commit_scan / _finish)
    CommitJob *cjob;               // [njobs] what the scan found out about a job
    int *chg;                      // [njobs][colcap] columns whose symbol for the row changes: y | old symbol << 24 | new symbol << 28
    int *evkey, *evdl;             // [njobs][EVCAP] structural events: 2y + 1 a column opens after y (+1), 2y column y is emptied (-1)
    int *insidx;                   // [njobs][Lmax] for a base that opens a column: its number among the row's new columns
    int *pair_cf, *pair_left;      // [njobs][njobs] (i, j > i): a change of job i lies in job j's interval; net columns job i opens left of it
    unsigned *ticket;              // arrivals at the end of k_commit_finish
};
#define NOT_MINE(JB, JOB) ((JB).split_world > 1 && (JOB) % (JB).split_world != (JB).split_rank)

// ---------------------------------------------------------------------------------------------
// wave / block primitives (gfx950: 64-wide waves, DPP row shifts and row broadcasts)
// ---------------------------------------------------------------------------------------------
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143
#define DPP_WAVE_SHR1 0x138

__device__ __forceinline__ int wave_incl_min(int v)
{
    int t;
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(1), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(2), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(4), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(8), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_BCAST15, 0xA, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_BCAST31, 0xC, 0xF, false); v = min(v, t);
    return v;
}
// prefix-min over lanes 0..15 only (wave totals of at most 16 waves)
__device__ __forceinline__ int row_incl_min(int v)
{
    int t;
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(1), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(2), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(4), 0xF, 0xF, false); v = min(v, t);
    t = __builtin_amdgcn_update_dpp(PWR_BIG, v, DPP_ROW_SHR(8), 0xF, 0xF, false); v = min(v, t);
    return v;
}
__device__ __forceinline__ unsigned wave_incl_add(unsigned v)
{
    unsigned t;
    t = __builtin_amdgcn_update_dpp(0u, v, DPP_ROW_SHR(1), 0xF, 0xF, false); v += t;
    t = __builtin_amdgcn_update_dpp(0u, v, DPP_ROW_SHR(2), 0xF, 0xF, false); v += t;
    t = __builtin_amdgcn_update_dpp(0u, v, DPP_ROW_SHR(4), 0xF, 0xF, false); v += t;
    t = __builtin_amdgcn_update_dpp(0u, v, DPP_ROW_SHR(8), 0xF, 0xF, false); v += t;
    t = __builtin_amdgcn_update_dpp(0u, v, DPP_ROW_BCAST15, 0xA, 0xF, false); v += t;
    t = __builtin_amdgcn_update_dpp(0u, v, DPP_ROW_BCAST31, 0xC, 0xF, false); v += t;
    return v;
}

// inclusive block prefix sum; sh needs NT/64 words; ends with a barrier so sh can be reused
template <int NT>
__device__ __forceinline__ unsigned block_incl_add(unsigned v, unsigned *sh, unsigned &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = wave_incl_add(v);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    unsigned wp = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        unsigned s = sh[w];
        wp += (w < wave) ? s : 0u;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return incl + wp;
}

template <int NT>
__device__ __forceinline__ unsigned block_min_u32(unsigned v, unsigned *sh)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = 0xffffffffu;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) r = min(r, sh[w]);
    __syncthreads();
    return r;
}
template <int NT>
__device__ __forceinline__ int block_max_i32(int v, int *sh)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = INT_MIN;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) r = max(r, sh[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ const int *cur_order(const DState &st)
{
    return st.hdr->cur ? st.order1 : st.order0;
}

// ---------------------------------------------------------------------------------------------
// gather: TheWay (PW:647-705) + Columns_Downdater (PW:1172-1201) into job-private DP inputs.
// One work-group per job.  The global state is NOT modified: the row's own symbols are
// subtracted from a private copy of the tallies, so many rows can be gathered from one state.
//
// Record of column y (16 B): x = S(y,0) | S(y,1)<<16, y = S(y,2) | S(y,3)<<16  (PW:243 Score),
//   z = G(y) = sum_{j=lo..y} S(j,4)   (mod 2^32; only differences inside one DP row are used),
//   w = max(S(y,5), S(y-1,5))  (PW:1507), or PWR_INF where PW:1505 forbids opening a column.
// ---------------------------------------------------------------------------------------------
#define GATHER_NT 1024
#define GATHER_G 16                // work-groups per job: the rows and the interval's columns are cut into that many shares
struct GatherPart { unsigned long long ucost, cells; unsigned sum4, maxS, lastcov, tag; };   // what a share contributes, tag = launch

// the job's row: the job-th row from next_row on that was not committed ahead of order already; -1: no such job in this batch
__device__ __forceinline__ int gather_row_of(const Hdr *hd, const int *bplan, int job, int *boff_out)
{
    int boff = 0;
    if (bplan[0] && job < PLAN_MAX) boff = bplan[1 + job];                       // picked by the batch before (k_commit_finish)
    else {
        const unsigned long long ah = hd->ahead;
        int cnt = -1;
        for (boff = 0; boff < 64; ++boff) if (!((ah >> boff) & 1ull) && ++cnt == job) break;
        if (boff == 64) boff = 64 + (job - cnt - 1);
    }
    *boff_out = boff;
    const int kk = hd->next_row + boff;
    if (hd->status != 0 || hd->need_grow || job >= hd->nb || kk >= hd->row_end) return -1;
    return kk;
}

// gather, step a: ordinals of the share's bases (TheWay, PW:647-705), row descriptors and reference cell count for them, the
// marks of the row's own symbols; share 0 writes the job's header.
__global__ __launch_bounds__(GATHER_NT) void k_gather_a(DState st, JobBufs jb, const int *jobrows)
{
    const int job = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    JobMeta *m = &jb.meta[job];
    const Hdr *hd = st.hdr;
    int boff;
    const int kk = gather_row_of(hd, st.bplan, job, &boff);
    if (g == 0) {
        // what the commit of this batch will note about the job (k_commit_scan) starts from nothing
        const int nj = (int)gridDim.x;
        if (tid == 0) { CommitJob z; z.nchg = z.nev = z.ndel = 0; z.first = 0x7fffffff; z.u0 = z.u1 = 0; z.scanned = 0; z.pad = 0; jb.cjob[job] = z; jb.chkdone[job] = 0; }
        for (int j = tid; j < nj; j += GATHER_NT) { jb.pair_cf[(size_t)job * nj + j] = 0; jb.pair_left[(size_t)job * nj + j] = 0; }
    }
    if (kk < 0) { if (tid == 0 && g == 0) m->active = 0; return; }
    const int k = jobrows[kk];
    const int L = st.rowlen[k];
    const int W = hd->W;
    if (L == 0) {
        if (tid == 0 && g == 0) { m->k = k; m->L = 0; m->ok = 1; m->W = W; m->nnew = 0; m->cells = 0; m->ver = hd->version; m->active = 1; m->off = boff; m->wide = 0; m->abort = 0; }
        return;
    }
    const long long off = st.rowoff[k];
    const int *order = cur_order(st);
    int *way = jb.way + (size_t)job * jb.Lmax;
    const int B = st.B, H = st.H;
    const int way0 = st.rank[st.pos[off]], wayL = st.rank[st.pos[off + L - 1]];
    const int a0 = max(0, way0 - H), aL = max(0, wayL - H);
    const int lo = max(0, a0 - 1), hi = min(W - 1, aL + B - 1);
    const int n = hi - lo + 1;
    if (g == 0 && tid < 64 && hd->jumpmask != 0ull) {
        // Rows that were committed AHEAD of this one although it was not in their batch (picked by k_commit_finish because their
        // intervals kept a wide gap from it): has the gap held?  What such a row's commit can have touched lies within rec[1] / rec[2]
        // columns of its first / last base -- as counted at its commit -- plus at most one column per structural event committed
        // since.  If this row's interval reaches that far, the two no longer commute and the state is not the reference's:
        // said loudly (never reached with the gaps and the event rates rows jump at; the option "plan_ahead" 0 rules it out).
        bool bad = false;
        if (tid > boff && ((hd->jumpmask >> tid) & 1ull)) {
            const int kkj = hd->next_row + tid;
            const int kj = jobrows[kkj], Lj = st.rowlen[kj];
            const long long oj = st.rowoff[kj];
            const int f = st.rank[st.pos[oj]], l = st.rank[st.pos[oj + Lj - 1]];
            const int *rec = st.bplan + JR_BASE + 4 * (kkj & 63);
            const int es = (int)((unsigned)hd->events_total - (unsigned)rec[0]);
            bad = !(hi + 2 < f - rec[1] - es || l + rec[2] + es < lo - 2);
        }
        if (__ballot(bad) != 0ull && tid == 0) atomicCAS(&st.hdr->status, 0, PWR_ERR_ORDER);
    }
    const int x0 = (int)((long long)L * g / GATHER_G), x1 = (int)((long long)L * (g + 1) / GATHER_G);
    // The marks of the row's own symbols (base + 1 where it has a base, 0 where it has '-', 7 in a blank run between two of
    // its segments): the share clears and sets the columns from its first base up to the next share's first base -- Way[] is
    // increasing, so the shares' column ranges tile the interval and nobody waits for anybody.
    uint8_t *mark = jb.mark + (size_t)job * jb.colcap;
    const int c0 = g == 0 ? lo : st.rank[st.pos[off + min(x0, L - 1)]], c1 = (g == GATHER_G - 1 || x1 >= L) ? hi + 1 : st.rank[st.pos[off + x1]];
    (void)n;
    for (int i = c0 - lo + tid; i < c1 - lo; i += GATHER_NT) mark[i] = 0;
    __syncthreads();
    unsigned long long mycells = 0;
    uint4 *desc = jb.desc + (size_t)job * jb.Lmax;
    const int NWg = jb.wpNW, MSg = jb.wpMS;
    for (int x = x0 + tid; x < x1; x += GATHER_NT) {
        const int wx = st.rank[st.pos[off + x]];
        way[x] = wx;
        mark[wx - lo] = (uint8_t)(st.seq[off + x] + 1);
        const int ax = max(0, wx - H), bx = min(B, W - ax);
        mycells += (unsigned long long)bx;                                          // cells of DP row x, PW:1496-1499
        // Row descriptors for the wave-pipeline fills: what every wave would otherwise recompute per DP row (anf < 2^24,
        // the row's base, and per wave 4 flag bits).  Wave w owns the macro-strip ms = ms_lo + ((w - ms_lo) mod NW) in row x:
        //   bit0 "ordinary row": the wave has work in rows x-1 and x on the same macro-strip, 0 < x < L-1, and the
        //        score left of the macro-strip is not the virtual extension G + Ptot(x-1) of PW:285-295
        //   bit1 needs the left neighbour's running minimum (its macro-strip is not the band's first)
        //   bit2 the score left of the macro-strip is the neighbour's boundary score of row x-1 (else INF, PW:276)
        //   bit3 the band ends in this macro-strip
        const int mlo = (ax - lo) / MSg, mhi = (ax + bx - 1 - lo) / MSg;
        int ap = 0, bp = 0, plo = 0, phi = -1;
        if (x > 0) {
            ap = max(0, st.rank[st.pos[off + x - 1]] - H); bp = min(B, W - ap);
            plo = (ap - lo) / MSg; phi = (ap + bp - 1 - lo) / MSg;
        }
        unsigned long long fl = 0;
        unsigned fl2 = 0;                                                           // waves 16..23
        for (int w = 0; w < NWg; ++w) {
            const int msw = mlo + (((w - mlo) % NWg) + NWg) % NWg;
            if (msw > mhi) continue;
            const int msp = plo + (((w - plo) % NWg) + NWg) % NWg;
            const bool ranp = x > 0 && msp == msw && msp <= phi;
            const int yq = lo + msw * MSg - 1;
            const unsigned kind = (x == 0 || yq < ap) ? 0u : (yq < ap + bp ? 1u : 2u);
            const unsigned bits = ((ranp && x < L - 1 && kind != 2u) ? 1u : 0u) | (msw > mlo ? 2u : 0u) | (kind == 1u ? 4u : 0u) | (msw == mhi ? 8u : 0u);
            if (w < 16) fl |= (unsigned long long)bits << (4 * w); else fl2 |= bits << (4 * (w - 16));
        }
        desc[x] = make_uint4((unsigned)ax | ((unsigned)st.seq[off + x] << 24), (unsigned)fl, (unsigned)(fl >> 32), fl2);
    }
    {
        // blank runs between the row's segments (rows read with interior blanks, until their first realignment)
        const int nbk = st.nbrk[k];
        const int *bxs = st.brkx + st.brkoff[k];
        for (int t = tid; t < nbk; t += GATHER_NT) {
            const int b = bxs[t];
            if (b >= x0 && b < x1)
                for (int y = st.rank[st.pos[off + b]] + 1; y < st.rank[st.pos[off + b + 1]]; ++y) mark[y - lo] = 7;
        }
    }
    for (int o = 32; o > 0; o >>= 1) mycells += __shfl_xor(mycells, o);
    __shared__ unsigned long long s_cells[GATHER_NT / 64];
    if ((tid & 63) == 0) s_cells[tid >> 6] = mycells;
    __syncthreads();
    if (tid == 0) {
        unsigned long long cs = 0;
        for (int w = 0; w < GATHER_NT / 64; ++w) cs += s_cells[w];
        jb.gpart[(size_t)job * GATHER_G + g].cells = cs;
        if (g == 0) {
            m->k = k; m->L = L; m->lo = lo; m->hi = hi; m->W = W; m->entry = -1; m->nnew = 0; m->abort = 0; m->active = 1; m->off = boff;
            m->ver = hd->version; m->slot_lo = order[lo]; m->slot_hi = order[hi]; m->ok = 1; m->changed = 0;
        }
    }
}

// The plan of a job's fill (one work-group): how many segments, where each starts to warm up, the cells it computes.
// Own parts and warm-ups start at multiples of 16 rows (the fill stores its record per 16 rows): a warm-up at the last one
// whose band lies at least warm_cols columns left of the own part's first band.  A row whose check failed is planned again
// with twice the warm-up, and in one piece if that fails too (Hdr::noseg_row / noseg_level).
__device__ void plan_segments(const DState &st, const JobBufs &jb, int job)
{
    __shared__ int s_x[SEG_MAX + 1], s_xb[SEG_MAX], s_S;
    __shared__ unsigned long long s_cells[SEG_MAX];
    const int tid = threadIdx.x;
    JobMeta *m = &jb.meta[job];
    SegDesc *sg = jb.seg + (size_t)job * SEG_MAX;
    if (!m->active || m->L <= 0) { if (tid < SEG_MAX) sg[tid].active = 0; return; }
    const int L = m->L, W = m->W, B = st.B, H = st.H;
    const int *way = jb.way + (size_t)job * jb.Lmax;
    __shared__ int s_warm;
    if (tid == 0) {
        int S = 1;
        const int level = st.hdr->noseg_row == m->k ? st.hdr->noseg_level : 0;     // how often this row's check has failed
        const int marked = jb.hard_rows ? (st.hard[m->k] > 0 ? 1 : 0) : 0;
        if (jb.seg_rows > 0 && level < 2) {
            // A launch ends with its longest chain of rows: own rows + warm-up of the job with the fewest segments per base.  The
            // chip holds about one worker wave per SIMD (seg_budget segments of NW waves) before the waves start to share issue
            // slots, so the batch's jobs are dealt the budget by their lengths: a long row next to two short ones is cut finer
            // than one of three long rows, and three short rows are cut finer than seg_rows asks for because there is room (every
            // job's plan sees the lengths of the others: the rows of a batch follow from the header).  Never finer than
            // seg_minrows own rows.  seg_budget 0: about seg_rows rows each, as many as that gives.
            const int natural = min((L + jb.seg_rows / 2) / jb.seg_rows, L / 128);
            S = natural;
            if (jb.seg_budget > 0) {
                const Hdr *hd = st.hdr;
                long long Lsum = 0;
                for (int j = 0; j < hd->nb; ++j) {
                    int bo;
                    const int kj = gather_row_of(hd, st.bplan, j, &bo);
                    if (kj >= 0) Lsum += st.rowlen[jb.rowids[kj]];
                }
                Lsum = max(Lsum, (long long)L);
                // (two alignment units of own rows at least: the own parts start at multiples of seg_align, and a segment
                // without rows of its own is none)
                S = min((int)((long long)jb.seg_budget * L / Lsum), L / max(max(16, jb.seg_minrows), 2 * jb.seg_align));
            }
        }
        S = max(1, min(S, jb.smax));
        s_S = S;
        // (a row whose check failed: the longest warm-up the steering allows, twice that if it was already there)
        const Hdr *hd = st.hdr;
        const bool steered = hd->warm_step > 0;
        s_warm = level == 1 ? ((steered && hd->warm_cur < jb.warm_cols) ? jb.warm_cols : 2 * jb.warm_cols) : (steered ? hd->warm_cur : jb.warm_cols);
        // "hard_rows" 1: a row whose check failed lately does not try the short warm-up again (2: only counted, test hook)
        const int longway = (marked && jb.hard_rows == 1 && level == 0 && steered) ? 1 : 0;
        if (longway) s_warm = min(max(s_warm, jb.warm_cols), s_warm + st.hard[m->k]);
        m->nseg = S; m->segfail = 0; m->level = level; m->hard = marked | (longway << 1);
    }
    if (tid < SEG_MAX) s_cells[tid] = 0;
    __syncthreads();
    const int S = s_S, warm = s_warm;
    if (tid <= S) s_x[tid] = tid == S ? L : (int)(((long long)L * tid / S) & ~(long long)(jb.seg_align - 1));   // (a multiple of 16: the record is stored per 16 rows)
    __syncthreads();
    // Where the own parts begin.  First in equal shares of the row; then -- "seg_balance" -- moved so that every segment has about
    // the same number of rows to run, warm-up included: a launch ends with its longest segment, the first one has no warm-up at
    // all, and a warm-up of so many COLUMNS is more rows where the row's bases sit closer together.  (The warm-ups of the moved
    // boundaries are looked up again; they differ a little from the ones the shares were cut by, which is all the same to the
    // results and nearly so to the balance.)
    for (int it = 0; it < 2; ++it) {
        if (it == 1) {
            if (!jb.seg_balance || S < 3) break;
            __shared__ int s_nx[SEG_MAX + 1], s_okb;
            if (tid == 0) {
                long long sumw = 0;
                for (int s2 = 1; s2 < S; ++s2) sumw += s_x[s2] - s_xb[s2];
                // (a row of the own part costs about 1.2 rows of a warm-up: it makes the record)
                const long long chain12 = (12LL * L + 10LL * sumw) / S;    // what every segment should cost, in tenths of a warm-up row
                const int al = jb.seg_align, minown = max(2 * al, 32);
                int x = 0, ok = 1;                                     // (x: the exact position; the boundaries are rounded down from it,
                s_nx[0] = 0;                                           // so the roundings do not add up in the last segment)
                for (int s2 = 0; s2 < S - 1; ++s2) {
                    x += max(minown, (int)((chain12 - 10LL * (s2 ? s_x[s2] - s_xb[s2] : 0)) / 12));
                    s_nx[s2 + 1] = min(x, L) & ~(al - 1);
                }
                s_nx[S] = L;
                for (int s2 = 0; s2 < S; ++s2) if (s_nx[s2 + 1] - s_nx[s2] < minown) ok = 0;   // (the last one takes what is left: too little -> equal shares)
                s_okb = ok;
            }
            __syncthreads();
            if (!s_okb) break;
            if (tid <= S) s_x[tid] = s_nx[tid];
            __syncthreads();
        }
        // xb of segment s: the largest multiple of 16 below x_s whose row sits at least `warm` columns left of row x_s (Way[]
        // is increasing).  Sixteen threads per segment, a 16-ary search: three dependent loads instead of twelve (this share
        // would otherwise be the one its kernel waits for).
        static_assert(SEG_MAX % (GATHER_NT / 16) == 0, "sixteen threads per segment, GATHER_NT / 16 segments per pass");
      for (int pass = 0; pass < SEG_MAX / (GATHER_NT / 16); ++pass) {
        if (pass * (GATHER_NT / 16) >= S) break;                 // (uniform)
        const int sgi = pass * (GATHER_NT / 16) + (tid >> 4), li = tid & 15;
        int lo_c = -1, hi_c = 0, lim = 0;                        // candidates 16 * c: c <= lo_c hold, c >= hi_c do not
        if (sgi > 0 && sgi < S) { const int xs = s_x[sgi]; lim = way[xs] - warm; hi_c = xs / 16; }
        for (int round = 0; round < 8; ++round) {                // (16^3 = 4096 candidates cover 35 000 rows; the bound is slack)
            const int span = hi_c - lo_c - 1;                    // undecided candidates
            const int step = (span + 15) / 16;                   // uniform over the 16 lanes of a segment
            const int cand = lo_c + (li + 1) * step;
            const bool test = sgi > 0 && sgi < S && span > 0 && cand < hi_c;
            const bool holds = test && way[16 * cand] <= lim;
            const unsigned long long bal = __ballot(holds);
            const unsigned mine = (unsigned)(bal >> (16 * ((tid & 63) >> 4))) & 0xffffu;   // this segment's 16 answers: a prefix of ones
            const int pt = __builtin_popcount(mine);
            if (span > 0) {
                const int nlo = pt > 0 ? lo_c + pt * step : lo_c;
                const int nhi = pt < 16 ? min(hi_c, lo_c + (pt + 1) * step) : hi_c;
                lo_c = nlo; hi_c = nhi;
            }
            if (__syncthreads_or(hi_c - lo_c - 1 > 0) == 0) break;
        }
        if (li == 0 && sgi < S) s_xb[sgi] = (sgi == 0 || lo_c < 0) ? 0 : 16 * lo_c;
      }
        __syncthreads();
    }
    __syncthreads();
    // cells of the rows [xb, xe): B each, less what the MSA's right edge cuts off the band (PW:1497) -- only the rows from
    // the first one whose band reaches it, a suffix of the row (Way[] is increasing): found by all threads at once
    __shared__ int s_xr, s_grow[SEG_MAX + 1];
    if (tid == 0) {
        s_xr = L;
        int grow = 0;
        for (int s2 = 0; s2 <= S; ++s2) { s_grow[s2] = grow; if (s2 < S) grow += s_x[s2 + 1] - s_xb[s2]; }
    }
    __syncthreads();
    {
        // first row x with max(0, way[x] - H) + B > W: every thread probes one of 1024 evenly spaced rows, then the rows of
        // the stretch in front of the first hit
        const int stride = L / GATHER_NT + 1;
        const int c = min(L - 1, tid * stride);
        if (max(0, way[c] - H) + B > W) atomicMin(&s_xr, c);
        __syncthreads();
        const int hit = s_xr;                                    // a probed row that qualifies (or L): the first one lies in (hit - stride, hit]
        __syncthreads();
        const int x2 = hit - stride + 1 + tid;
        if (tid < stride && x2 >= 0 && x2 < hit && max(0, way[x2] - H) + B > W) atomicMin(&s_xr, x2);
        __syncthreads();
    }
    const int xr = s_xr;
    for (int x = xr + tid; x < L; x += GATHER_NT) {
        const unsigned long long cut = (unsigned long long)(B - min(B, W - max(0, way[x] - H)));
        if (cut) for (int s2 = S - 1; s2 >= 0 && s_x[s2 + 1] > x; --s2) if (s_xb[s2] <= x) atomicAdd(&s_cells[s2], cut);
    }
    __syncthreads();
    if (tid < SEG_MAX) {
        const int s2 = tid;
        SegDesc d;
        d.job = job; d.s = s2; d.active = s2 < S ? 1 : 0;
        d.xb = d.xown = d.xe = 0; d.fin = 0; d.grow0 = 0; d.cells = 0;
        if (s2 < S) {
            d.xb = s_xb[s2]; d.xown = s_x[s2]; d.xe = s_x[s2 + 1]; d.fin = s2 == S - 1 ? 1 : 0;
            d.grow0 = s_grow[s2];
            d.cells = (unsigned long long)(d.xe - d.xb) * (unsigned long long)B - s_cells[s2];
        }
        sg[s2] = d;
    }
}

// gather, step c: Columns_Downdater (PW:1172-1201) into job-private DP inputs for the share's columns.  The prefix sums G run
// over the whole interval: every share first publishes the sum over its own columns (with the launch's tag), then adds up
// the shares before it -- they only depend on their own columns, so nobody waits long.  The last share finishes the header.
__global__ __launch_bounds__(GATHER_NT) void k_gather_c(DState st, JobBufs jb)
{
    __shared__ unsigned sh[GATHER_NT / 64];
    __shared__ unsigned s_cov[GATHER_NT + 1];
    __shared__ unsigned long long s_u[GATHER_NT / 64];
    __shared__ unsigned s_carry, s_covl;
    const int job = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    if (g == GATHER_G) { plan_segments(st, jb, job); return; }                       // (the share after the last one plans the job's fill)
    JobMeta *m = &jb.meta[job];
    if (!m->active || m->L <= 0) return;
    const int L = m->L, lo = m->lo, hi = m->hi, W = m->W, B = st.B;
    const int n = hi - lo + 1;
    const int *order = cur_order(st);
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const int way0 = way[0], wayL = way[L - 1];
    const uint8_t *mark = jb.mark + (size_t)job * jb.colcap;
    int4 *rec2 = jb.rec2 + (size_t)job * jb.colcap * 2;
    GatherPart *part = jb.gpart + (size_t)job * GATHER_G;
    const unsigned tag = jb.gather_tag;
    const int i0 = (int)((long long)n * g / GATHER_G), i1 = (int)((long long)n * (g + 1) / GATHER_G);
    auto tally_of = [&](int y, uint32_t *w, unsigned long long *uc) {
        const Tally t = st.tally[order[y]];
#pragma unroll
        for (int b = 0; b < 6; ++b) w[b] = t.w[b];
        if (y >= way0 && y <= wayL) {                                                // the row's own symbol: a base, '-' or (7) blank
            const int mk = mark[y - lo];
            const int own = mk == 7 ? 5 : (mk ? mk - 1 : 4);
#pragma unroll
            for (int b = 0; b < 6; ++b) w[b] -= (own != 5 && b != own) ? 1u : 0u;
            if (uc) {
#pragma unroll
                for (int b = 0; b < 5; ++b) *uc += (b == own) ? w[b] : 0u;
            }
        }
    };
    // pass 1: this share's sum of S(.,4).  The tallies it reads (two dependent loads per column) are kept in registers for
    // pass 2, for the first GC_K columns of every thread -- all of them unless the interval is longer than 49 000 columns
    constexpr int GC_K = 6;
    uint32_t cw[GC_K][6];
    unsigned mysum = 0;
    unsigned long long ucost = 0;                                                    // cost of the row where it stands now: an upper bound of the optimum
#pragma unroll
    for (int it = 0; it < GC_K; ++it) {
        const int i = i0 + tid + it * GATHER_NT;
#pragma unroll
        for (int b = 0; b < 6; ++b) cw[it][b] = 0;
        if (i < i1) { tally_of(lo + i, cw[it], &ucost); mysum += cw[it][4]; }
    }
    for (int i = i0 + tid + GC_K * GATHER_NT; i < i1; i += GATHER_NT) { uint32_t w[6]; tally_of(lo + i, w, nullptr); mysum += w[4]; }
    for (int o = 32; o > 0; o >>= 1) mysum += __shfl_xor(mysum, o);
    if ((tid & 63) == 0) sh[tid >> 6] = mysum;
    __syncthreads();
    if (tid == 0) {
        unsigned tot = 0;
        for (int w = 0; w < GATHER_NT / 64; ++w) tot += sh[w];
        __hip_atomic_store(&part[g].sum4, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part[g].tag, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < 64) {
        // the shares before this one, one lane each (one thread asking them in turn paid a round trip per share: the last
        // share sixteen of them, on the critical path of every batch)
        unsigned mine = 0;
        if (tid < g) {
            while (__hip_atomic_load(&part[tid].tag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != tag) __builtin_amdgcn_s_sleep(1);
            mine = __hip_atomic_load(&part[tid].sum4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if (tid == 0) s_carry = mine;
    } else if (tid == 64) {
        uint32_t wl[6] = {0, 0, 0, 0, 0, 0};
        if (i0 > 0) tally_of(lo + i0 - 1, wl, nullptr);                              // coverage of the column left of the share
        s_covl = wl[5];
    }
    __syncthreads();
    // pass 2: the records
    unsigned carry = s_carry, maxS = 0;
    if (tid == 0) s_cov[0] = s_covl;
    __syncthreads();
    int it2 = 0;
    for (int base = i0; base < i1; base += GATHER_NT, ++it2) {
        const int i = base + tid;
        const bool valid = i < i1;
        const int y = lo + i;
        uint32_t w[6] = {0, 0, 0, 0, 0, 0};
        if (it2 < GC_K) {
#pragma unroll
            for (int k = 0; k < GC_K; ++k)
                if (it2 == k) {
#pragma unroll
                    for (int b = 0; b < 6; ++b) w[b] = cw[k][b];
                }
        } else if (valid) tally_of(y, w, &ucost);
        unsigned tot;
        const unsigned gin = block_incl_add<GATHER_NT>(w[4], sh, tot);               // barriers inside
        s_cov[tid + 1] = w[5];
        __syncthreads();
        const unsigned covl = s_cov[tid];
        __syncthreads();
        if (tid == GATHER_NT - 1) s_cov[0] = w[5];
        if (valid) {
            const unsigned upc = (y == 0 || y == W - 1) ? PWR_INF : max(w[5], covl);
            const int gq = (int)(carry + gin);
            rec2[2 * i] = make_int4((int)w[0] - gq, (int)w[1] - gq, (int)w[2] - gq, (int)w[3] - gq);
            rec2[2 * i + 1] = make_int4((int)(upc == PWR_INF ? PWR_INF - 1u : upc) - gq, gq, (int)PWR_INF - gq, 0);   // INF-1: pm + up stays below 2^31
            maxS = max(maxS, max(max(w[0], w[1]), max(max(w[2], w[3]), max(w[4], w[5]))));
        }
        carry += tot;
        __syncthreads();
    }
    const unsigned mx = (unsigned)(~block_min_u32<GATHER_NT>(~maxS, sh));
    for (int o = 32; o > 0; o >>= 1) ucost += __shfl_xor(ucost, o);
    if ((tid & 63) == 0) s_u[tid >> 6] = ucost;
    __syncthreads();
    if (tid == 0) {
        unsigned long long U = 0;
        for (int w = 0; w < GATHER_NT / 64; ++w) U += s_u[w];
        __hip_atomic_store(&part[g].ucost, U, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part[g].maxS, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part[g].lastcov, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);   // "second half done"
    }
    if (g == GATHER_G - 1 && tid < 64) {
        // 32-bit range.  The row's present placement is a path inside the band, so the optimum and every
        // cell on an optimal path are <= U = its cost; larger values may saturate at PWR_INF without
        // touching any test the traceback makes.  Offsets of at most (2B + slack) * maxS are added on top.
        // (all shares asked at once, one lane each)
        unsigned long long Ut = 0, cs = 0;
        unsigned mxt = 0;
        if (tid < GATHER_G) {
            while (__hip_atomic_load(&part[tid].lastcov, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != tag) __builtin_amdgcn_s_sleep(1);
            Ut = __hip_atomic_load(&part[tid].ucost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mxt = __hip_atomic_load(&part[tid].maxS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cs = part[tid].cells;                                                    // (written by the launch before)
        }
        for (int o = 32; o > 0; o >>= 1) { Ut += __shfl_xor(Ut, o); cs += __shfl_xor(cs, o); mxt = max(mxt, (unsigned)__shfl_xor((int)mxt, o)); }
        if (tid == 0) {
            const unsigned long long bound = Ut + (unsigned long long)mxt * (unsigned long long)(2 * B + 4096);
            m->maxS = mxt; m->cells = cs;
            // the wave pipeline works with absolute prefix sums G: their total (= bases in the interval) must stay below 2^29
            m->wide = (jb.force64 || !(bound < (unsigned long long)PWR_INF && carry < (1u << 29))) ? 1 : 0;   // -> k_fill64
            if (m->wide) st.hdr->need64 = 65;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fill v2: the wave pipeline in lock-step rounds (one s_barrier per round instead of polled mailboxes),
// with the per-cell and per-row work cut down.
//   * prefix sums G are absolute (their total is the number of bases in the interval, < 2^29, checked by
//     the gather), so the per-column constants S_b - G, up - G, INF - G are precomputed once per column
//     and a candidate is  tg = min3(pm1 + (S_b - G), pm + (up - G), INF - G)  -- three VALU ops;
//   * the row's base selects one of four straight-line copies of the cell loop (no per-cell select);
//   * traceback bits are OR-ed in at their final position; rows without work for a wave cost no VALU;
//   * a wave may retire up to V2_R rows per round (its left neighbour is that far ahead), so the
//     barrier is amortised; all control state is kept wave-uniform (SGPRs, scalar branches).
// ---------------------------------------------------------------------------------------------
#define V2_D 128                                     // mailbox depth (rows); a wave is never more than V2_R rows ahead of its reader
#define V2_PD 512
#define V2_R 64
#define V2_SPINS 256
#define FBIG 0x3fffffff                              // neutral element of the fast path's min-scan (G + FBIG stays below 2^31)
#define UNI(v) __builtin_amdgcn_readfirstlane(v)

// shift a traceback-bit accumulator left by one and insert the lane's bit of MASK (a v_cmp result): one VALU op
__device__ __forceinline__ unsigned acc_push(unsigned acc, unsigned long long mask)
{
    unsigned long long carry_out;
    asm("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(acc), "=s"(carry_out) : "s"(mask));
    return acc;
}
#define ICMP_SGE 39
#define ICMP_SLT 40
#define ICMP_SLE 41

// records of macro-strip MSX: the four substitution columns S_b - G go to this wave's LDS table SLOT (read back
// per DP row with the row's base as the index), the rest stays in registers
#define V2_LOAD(MSX, SLOT, AU, AG, AI, GL)                                                       \
    {                                                                                            \
        _Pragma("unroll") for (int i = 0; i < C; ++i) {                                          \
            const int y_ = lo + (MSX) * MS + lc + i;                                             \
            int4 p_ = make_int4(PWR_BIG / 2, PWR_BIG / 2, PWR_BIG / 2, PWR_BIG / 2);             \
            int4 q_ = make_int4(PWR_BIG / 2, 0, PWR_BIG / 2, 0);                                 \
            if (y_ <= hi) { p_ = rec2[2 * (y_ - lo)]; q_ = rec2[2 * (y_ - lo) + 1]; }            \
            ldsS[wave][SLOT][0][lc + i] = p_.x; ldsS[wave][SLOT][1][lc + i] = p_.y;              \
            ldsS[wave][SLOT][2][lc + i] = p_.z; ldsS[wave][SLOT][3][lc + i] = p_.w;              \
            AU[i] = q_.x; AG[i] = q_.y; AI[i] = q_.z;                                            \
        }                                                                                        \
        const int yq_ = lo + (MSX) * MS - 1;                                                     \
        GL = (yq_ >= lo && yq_ <= hi) ? UNI(rec2[2 * (yq_ - lo) + 1].y) : 0;                     \
    }

template <int NW, int C>
__global__ __launch_bounds__(NW * 64) void k_fill_v2(DState st, JobBufs jb)   // (jobs flagged wide are left to k_fill64)
{
    constexpr int MS = 64 * C, RS = NW * MS;
    // What lane 63 of a wave publishes per DP row.  Every item is one 64-bit word {value, row + 1}, stored and loaded
    // with single 8-byte LDS accesses (relaxed atomics, so the compiler can neither split nor merge them): the row
    // number makes it self-validating, a reader needs no other signal.  Behind the real slots of each array there
    // is one private dump slot per lane, so that a store is steered by its index alone (lane 63 to the real slot,
    // the others to their dump slot) instead of by EXEC:
    //   mbQ[2 * (w * V2_D + x % V2_D) + 0]  P_end of row x of wave w (the running minimum its right neighbour continues)
    //   mbQ[2 * (w * V2_D + x % V2_D) + 1]  M_last, the score of its last column
    //   ptQ[x % V2_PD]                      Ptot, the minimum of the whole row x
    constexpr int MBDUMP = NW * V2_D, PTDUMP = V2_PD;
    __shared__ unsigned long long mbQ[2 * (MBDUMP + NW * 64)];
    __shared__ unsigned long long ptQ[PTDUMP + NW * 64];
    __shared__ __attribute__((aligned(16))) int ldsS[NW][2][4][MS];
    __shared__ int rdone[NW];                       // round + 1 once wave w has left that round
    __shared__ int s_done;
#define LD64(REF) __hip_atomic_load(&(REF), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LD32LO(REF) __hip_atomic_load((unsigned *)&(REF), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)   /* value half */
#define ST64(REF, VAL, TAG) __hip_atomic_store(&(REF), ((unsigned long long)(unsigned)(TAG) << 32) | (unsigned)(VAL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define MBP(W_, X_) mbQ[2 * ((W_) * V2_D + ((X_) & (V2_D - 1)))]
#define MBM(W_, X_) mbQ[2 * ((W_) * V2_D + ((X_) & (V2_D - 1))) + 1]
#define PTB(X_) ptQ[(X_) & (V2_PD - 1)]

    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = UNI(tid >> 6);
    JobMeta *m = &jb.meta[job];
    const int L = UNI(m->L);
    if (jb.gate_v2 && st.hdr->fallback <= 0) return;                              // only the stand-in for k_fill_v3 here
    if (!m->active || L <= 0 || !m->ok || m->wide || NOT_MINE(jb, job)) return;
    const unsigned long long t_clk0 = __builtin_amdgcn_s_memtime(), t_real0 = __builtin_amdgcn_s_memrealtime();
    for (int i = tid; i < 2 * (MBDUMP + NW * 64); i += NW * 64) mbQ[i] = 0;
    for (int i = tid; i < PTDUMP + NW * 64; i += NW * 64) ptQ[i] = 0;
    if (tid < NW) rdone[tid] = 0;
    if (tid == 0) s_done = 0;
    __syncthreads();

    const int lo = UNI(m->lo), hi = UNI(m->hi), W = UNI(m->W), B = st.B, H = st.H;
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const uint8_t *seq = st.seq + st.rowoff[UNI(m->k)];
    const int4 *rec2 = jb.rec2 + (size_t)job * jb.colcap * 2;
    uint32_t *dirs = jb.dirs + (size_t)job * jb.dirstride;
    unsigned *lastM = jb.lastM + (size_t)job * jb.NC;
    const int wl = (wave + NW - 1) % NW;
    const int lc = lane * C;
    const int mb_dump = MBDUMP + wave * 64 + lane, pt_dump = PTDUMP + wave * 64 + lane;   // where lanes 0..62 "publish" to

    // per-column constants of the current (ug, gg, ig) and the prefetched (nu, ng, ni) macro-strip
    int ug[C], gg[C], ig[C];
    int nu[C], ng[C], ni[C];
    int gleft = 0, gleftn = 0;
    int ms = wave, msn = wave + NW;
    int cs = 0;                                                     // LDS table slot of the current macro-strip
    V2_LOAD(ms, 0, ug, gg, ig, gleft)
    V2_LOAD(msn, 1, nu, ng, ni, gleftn)

    unsigned Mprev[C], accA[C], accC[C];
#pragma unroll
    for (int i = 0; i < C; ++i) { Mprev[i] = 0; accA[i] = accC[i] = 0; }
    int gacc = -1, nacc = 0;                                // 16-row group the accumulators belong to, rows pushed so far
    int ran_prev = 0, finished = 0;
    int x = 0, blk = 0;
    int wcur = way[min(lane, L - 1)], scur = seq[min(lane, L - 1)];
    int wnxt = way[min(64 + lane, L - 1)], snxt = seq[min(64 + lane, L - 1)];
    // row descriptors of the gather (64 rows per register, like Way[]): anf, Bx | base << 16, this wave's flags
    const uint4 *desc = jb.desc + (size_t)job * jb.Lmax;
    const int fsh = 4 * (wave & 7);
    const unsigned *descw = (const unsigned *)desc + 1 + (wave >> 3);      // this wave's flag word of a descriptor
    unsigned dca = desc[min(lane, L - 1)].x, dcf = descw[4 * min(lane, L - 1)] >> fsh;
    unsigned dna = desc[min(64 + lane, L - 1)].x, dnf = descw[4 * min(64 + lane, L - 1)];      // (shifted when the block becomes current)
    int a = max(0, __builtin_amdgcn_readlane(wcur, 0) - H), a_prev = 0, Bx_prev = 0;
    int sx = __builtin_amdgcn_readlane(scur, 0);
    const int max_rounds = 4 * L + 64 * NW + 1024;
    int round = 0;

    // the accumulators take one bit per DP row, most significant first; rows of the group this wave had no
    // work in are zeros
#define V2_ALIGN_ACC(WANT)                                                                       \
    if (nacc != (WANT)) {                                                                        \
        const int sh_ = (WANT) - nacc;                                                           \
        _Pragma("unroll") for (int i = 0; i < C; ++i) { accA[i] <<= sh_; accC[i] <<= sh_; }      \
        nacc = (WANT);                                                                           \
    }
#define V2_FLUSH()                                                                               \
    if (gacc >= 0) {                                                                             \
        V2_ALIGN_ACC(16)                                                                         \
        uint32_t *d_ = dirs + (size_t)gacc * RS + (size_t)wave * MS + (size_t)lc;                \
        _Pragma("unroll") for (int i = 0; i < C; ++i) { d_[i] = accA[i] | (accC[i] << 16); accA[i] = accC[i] = 0; } \
        gacc = -1; nacc = 0;                                                                     \
    }
#define V2_NEXT_ROW()                                                                            \
    {                                                                                            \
        a_prev = a; Bx_prev = Bx;                                                                \
        ++x;                                                                                     \
        if (x < L) {                                                                             \
            if ((x >> 6) != blk) {                                                               \
                blk = x >> 6;                                                                    \
                wcur = wnxt; scur = snxt; dca = dna; dcf = dnf >> fsh; \
                wnxt = way[min(x + 64 + lane, L - 1)];                                           \
                snxt = seq[min(x + 64 + lane, L - 1)];                                           \
                dna = desc[min(x + 64 + lane, L - 1)].x; dnf = descw[4 * min(x + 64 + lane, L - 1)]; \
            }                                                                                    \
            a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);                             \
            sx = __builtin_amdgcn_readlane(scur, x & 63);                                        \
        } else {                                                                                 \
            finished = 1;                                                                        \
            V2_FLUSH()                                                                           \
            if (lane == 0) atomicAdd(&s_done, 1);                                                \
        }                                                                                        \
    }

    for (; round < max_rounds; ++round) {
        int budget = V2_R;
        while (budget > 0) {
            // loop-carried control state is wave-uniform; say so, so it lives in SGPRs and branches are scalar
            finished = UNI(finished);
            if (finished) break;
            ran_prev = UNI(ran_prev); gacc = UNI(gacc); nacc = UNI(nacc); blk = UNI(blk); ms = UNI(ms); cs = UNI(cs); gleft = UNI(gleft);
            // ---- fast path: a run of ordinary rows (flagged by the gather: same macro-strip in the band as in the
            //      row before, not the first / last row) of the current 16-row group and 64-row block, as one
            //      straight-line loop body.  Everything the left neighbour posted stays in VGPRs (an LDS read gives
            //      every lane the same value), lane 63 publishes by index, and the row's substitution column comes
            //      from the LDS table -- no EXEC changes, no scalar round trips, one exit test.
            bool not_ready = false;
            if (ran_prev) {
                if ((x >> 4) != gacc) { V2_FLUSH() gacc = x >> 4; }
                unsigned mlast_v = (unsigned)LD64(MBM(wl, x - 1));                   // M_last(x-1) of the left neighbour
                const int y0f = lo + ms * MS;
                const int rel00 = y0f + lc;
                // rows this loop may take: up to the last but one of the 64-row block (the general path rotates the
                // per-block registers), not the last row
                const int xstop = UNI(min(L - 1, ((blk + 1) << 6) - 1));
                const int x_in = x;
                V2_ALIGN_ACC(x & 15)
                // the substitution column of the NEXT row is fetched from the LDS table while the current row is computed
                unsigned db = (unsigned)__builtin_amdgcn_readlane((int)dca, x & 63);        // {anf, base << 24} of row x
                int sgr[C];
#pragma unroll
                for (int i = 0; i < C; ++i) sgr[i] = ldsS[wave][cs][min(db >> 24, 3u)][lc + i];
                // have the loads above land before the loop, so that the waits inside it are the steady-state ones
#pragma unroll
                for (int i = 0; i < C; ++i) asm volatile("" : "+v"(sgr[i]));
                asm volatile("" : "+v"(mlast_v));
                int cnt = min(budget, xstop - x) - 1;                                // rows the loop may still take, less one
                int bail = 0;
                // One ordinary row.  fl = its flags, dbn = the {Bx, base} descriptor word of the row after it.
                auto fast_row = [&](const int fl, const unsigned dbn) __attribute__((always_inline)) {
                    const int af = (int)(db & 0xffffffu);
                    const int Bxf = min(B, W - af);
                    a_prev = af; Bx_prev = Bxf;                                      // for the general path, should it take the next row
                    db = dbn;
                    const int Mleft_v = (fl & 4) ? (int)mlast_v : (int)PWR_INF;
                    const int pm1_0 = __builtin_amdgcn_update_dpp(Mleft_v, (int)Mprev[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);
                    const int rel0 = rel00 - af;
                    int tg[C];
                    int run = FBIG;
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const int pm1 = i ? (int)Mprev[i > 0 ? i - 1 : 0] : pm1_0;
                        const int d = pm1 + sgr[i];
                        const int u = (int)Mprev[i] + ug[i];
                        accC[i] = acc_push(accC[i], __builtin_amdgcn_sicmp(d, u, ICMP_SLE));
                        const int t3 = min(min(d, u), ig[i]);
                        tg[i] = ((unsigned)(rel0 + i) < (unsigned)Bxf) ? t3 : FBIG;
                        run = min(run, tg[i]);
                    }
                    // The left neighbour's words of this row are only needed after the scan: ask for them now, and if they
                    // are not there yet wait for them THERE -- the neighbour is then half a row ahead, not a whole one.
                    // M first: it is stored last, so its row number vouches for P_end as well (of which only the value
                    // half is read).
                    unsigned long long fM = LD64(MBM(wl, x));
                    unsigned fP = LD32LO(MBP(wl, x));
                    __builtin_amdgcn_sched_barrier(0);
                    // The scan: six dependent DPP steps, each of which must be two issue slots behind the one before.
                    // Those slots are filled by hand with work that does not depend on it: the fetch of the next row's
                    // substitution column, and where / under which row number this row will be published.
#define V2_SCAN_STEP(CTRL, RMASK) { const int t_ = __builtin_amdgcn_update_dpp(PWR_BIG, incl, CTRL, RMASK, 0xF, false); incl = min(incl, t_); }
#define V2_FENCE() __builtin_amdgcn_sched_barrier(0)
                    int incl = run;
                    V2_SCAN_STEP(DPP_ROW_SHR(1), 0xF) V2_FENCE();
                    const unsigned sxn = min(db >> 24, 3u);
                    V2_FENCE(); V2_SCAN_STEP(DPP_ROW_SHR(2), 0xF) V2_FENCE();
                    const int *const srow = &ldsS[wave][cs][sxn][lc];
                    const int qs = wave * V2_D + (x & (V2_D - 1));
                    V2_FENCE(); V2_SCAN_STEP(DPP_ROW_SHR(4), 0xF) V2_FENCE();
#pragma unroll
                    for (int i = 0; i < C; ++i) sgr[i] = srow[i];
                    int qi = lane == 63 ? qs : mb_dump;
                    asm volatile("" : "+v"(qi));                                     // (keeps the select in this slot)
                    V2_FENCE(); V2_SCAN_STEP(DPP_ROW_SHR(8), 0xF) V2_FENCE();
                    unsigned qoff = (unsigned)qi * 16u;                              // byte offset of the two words in mbQ
                    asm volatile("" : "+v"(qoff));
                    unsigned long long *const qp = (unsigned long long *)((char *)mbQ + qoff);
                    V2_FENCE(); V2_SCAN_STEP(DPP_ROW_BCAST15, 0xA) V2_FENCE();
                    const unsigned long long tagw = (unsigned long long)(unsigned)(x + 1) << 32;
                    asm volatile("" :: "v"((unsigned)(tagw >> 32)));
                    V2_FENCE(); V2_SCAN_STEP(DPP_ROW_BCAST31, 0xC) V2_FENCE();
#undef V2_SCAN_STEP
#undef V2_FENCE
                    const int excl = __builtin_amdgcn_update_dpp(PWR_BIG, incl, DPP_WAVE_SHR1, 0xF, 0xF, false);
                    if (fl & 2) {
                        const unsigned tagx = (unsigned)(x + 1);
#define V2_BOTH_THERE() (UNI((unsigned)(fM >> 32)) == tagx)
                        if (!V2_BOTH_THERE()) {
                            // bounded; gives up at once when the neighbour has left the round (rdone is stored after its
                            // last entry, and LDS keeps one wave's stores in order)
                            for (int spin = 0; spin < V2_SPINS; ++spin) {
                                const int rd = UNI(__hip_atomic_load(&rdone[wl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                                __builtin_amdgcn_s_sleep(1);
                                fM = LD64(MBM(wl, x)); fP = LD32LO(MBP(wl, x));
                                if (V2_BOTH_THERE() || rd == round + 1) break;
                            }
                            if (!V2_BOTH_THERE()) bail = 1;
                        }
#undef V2_BOTH_THERE
                    }
                    if (!bail) {
                        const int P_in_v = (fl & 2) ? (int)fP : PWR_BIG;
                        const int P_end_v = min(P_in_v, incl);                       // lane 63: the row's running minimum so far
                        // cells left of the band come before its first cell in scan order, so their p is still the
                        // neutral element FBIG = 2^30 - 1 and G + p lands at or above INF by itself; the min keeps it there
                        int p = min(min(P_in_v, excl), FBIG);
#pragma unroll
                        for (int i = 0; i < C; ++i) {
                            accA[i] = acc_push(accA[i], __builtin_amdgcn_sicmp(tg[i], p, ICMP_SGE));
                            p = min(p, tg[i]);
                            Mprev[i] = min((unsigned)(gg[i] + p), PWR_INF);
                        }
                        mlast_v = (unsigned)fM;                                      // valid whenever the next row needs it
                        ++x; --cnt;
                        __hip_atomic_store(qp, tagw | (unsigned)P_end_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(qp + 1, tagw | Mprev[C - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (fl & 8)                                                  // the band ends in this macro-strip
                            ST64(ptQ[lane == 63 ? ((x - 1) & (V2_PD - 1)) : pt_dump], P_end_v, x);
                        if ((x & 15) == 0) {                                         // the 16-row group is complete
                            uint32_t *d_ = dirs + (size_t)gacc * RS + (size_t)wave * MS + (size_t)lc;
#pragma unroll
                            for (int i = 0; i < C; ++i) { d_[i] = accA[i] | (accC[i] << 16); accA[i] = accC[i] = 0; }
                            gacc = x >> 4;
                        }
                    } else {
                        cnt = -1;                                // the neighbour will not post row x in this round
                    }
                };
                while (true) {
                    x = UNI(x); cnt = UNI(cnt); gacc = UNI(gacc); db = UNI(db); bail = UNI(bail);
                    const int fl = __builtin_amdgcn_readlane((int)dcf, x & 63);
                    // one exit test (sign bits): no rows left (or the row before gave up) / not an ordinary row (bit 0 clear)
                    if ((cnt | ~(fl << 31)) < 0) break;
                    fast_row(fl, (unsigned)__builtin_amdgcn_readlane((int)dca, (x + 1) & 63));
                }
                // The last row of a 64-row block, if it is an ordinary one as well: its successor's descriptor is in the
                // registers of the next block, which then become the current ones (as in V2_NEXT_ROW).
                if (!bail && budget - (x - x_in) > 0 && (x & 63) == 63 && x < L - 1) {
                    const int fl = __builtin_amdgcn_readlane((int)dcf, 63);
                    if (fl & 1) {
                        cnt = 0;
                        fast_row(fl, (unsigned)__builtin_amdgcn_readlane((int)dna, 0));
                        if (!bail) {
                            blk = x >> 6;
                            wcur = wnxt; scur = snxt; dca = dna; dcf = dnf >> fsh;
                            wnxt = way[min(x + 64 + lane, L - 1)];
                            snxt = seq[min(x + 64 + lane, L - 1)];
                            dna = desc[min(x + 64 + lane, L - 1)].x; dnf = descw[4 * min(x + 64 + lane, L - 1)];
                        }
                    }
                }
                budget -= x - x_in;
                if (bail) {                                      // take the unfinished row back and leave the round
#pragma unroll
                    for (int i = 0; i < C; ++i) accC[i] >>= 1;
                    not_ready = true;
                }
                if (x != x_in) {                                                     // resynchronise the general path's row state
                    nacc = x & 15;
                    a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
                    sx = __builtin_amdgcn_readlane(scur, x & 63);
                    if (!not_ready && budget > 0) continue;                          // more ordinary rows, most likely
                }
            }
            if (not_ready || budget <= 0) break;
            x = UNI(x); ms = UNI(ms); msn = UNI(msn); a = UNI(a); a_prev = UNI(a_prev); Bx_prev = UNI(Bx_prev);
            sx = UNI(sx); gacc = UNI(gacc); nacc = UNI(nacc); blk = UNI(blk); gleft = UNI(gleft); gleftn = UNI(gleftn); ran_prev = UNI(ran_prev); cs = UNI(cs);
            const int Bx = min(B, W - a);
            const int ms_lo = (a - lo) / MS, ms_hi = (a + Bx - 1 - lo) / MS;
            if (ms < ms_lo) {
                // the macro-strip dropped out of the band for good: take over the one NW further right
                ms += NW;
                if (ms == msn) {
#pragma unroll
                    for (int i = 0; i < C; ++i) { ug[i] = nu[i]; gg[i] = ng[i]; ig[i] = ni[i]; }
                    gleft = gleftn;
                    cs ^= 1;
                } else {
                    while (ms < ms_lo) ms += NW;
                    V2_LOAD(ms, cs, ug, gg, ig, gleft)
                }
                msn = ms + NW;
                V2_LOAD(msn, cs ^ 1, nu, ng, ni, gleftn)
                ran_prev = 0;
                continue;
            }
            if (ms > ms_hi) {                               // no work for this wave in row x
                ran_prev = 0;
                V2_NEXT_ROW()
                continue;
            }
            // ---- inputs of (x, ms): written by the left neighbour before the last barrier?
            const int y0 = lo + ms * MS;
            const int yq = y0 - 1;
            const bool needP = ms > ms_lo;
            const bool needM = x > 0 && yq >= a_prev && yq < a_prev + Bx_prev;
            const bool needT = x > 0 && ((yq >= a_prev + Bx_prev) || !ran_prev);
            // bounded wait: the neighbour is usually within a row of posting what is missing; give up at once when it
            // has left the round (rdone is stored after its last entry, LDS keeps one wave's stores in order)
            unsigned ePx = 0, ePy = 0, eMy = 0, eTx = 0;
            bool ready = false;
            for (int spin = 0; spin < V2_SPINS; ++spin) {
                const int rd = UNI(__hip_atomic_load(&rdone[wl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (spin) __builtin_amdgcn_s_sleep(1);
                const unsigned long long eP = LD64(MBP(wl, x)), eQ = LD64(MBM(wl, x));   // P_end(x), M_last(x) of the left neighbour
                const unsigned long long eM = LD64(MBM(wl, x - 1)), eT = LD64(PTB(x - 1));
                ePx = UNI((unsigned)eP); ePy = UNI((unsigned)eQ);
                eMy = UNI((unsigned)eM);
                eTx = UNI((unsigned)eT);
                ready = (!needP || (UNI((unsigned)(eP >> 32)) == (unsigned)(x + 1) && UNI((unsigned)(eQ >> 32)) == (unsigned)(x + 1))) &&
                        (!needM || UNI((unsigned)(eM >> 32)) == (unsigned)x) && (!needT || UNI((unsigned)(eT >> 32)) == (unsigned)x);
                if (ready || rd == round + 1) break;
            }
            if (!ready) break;
            --budget;
            int Mleft = (int)PWR_INF;
            if (x == 0) Mleft = 0;
            else if (yq < a_prev) Mleft = (int)PWR_INF;                              // PW:276
            else if (needM) Mleft = (int)eMy;
            else Mleft = gleft + (int)eTx;                                           // PW:285-295
            const int P_in = needP ? (int)ePx : PWR_BIG;
            if (x > 0 && !ran_prev) {
#pragma unroll
                for (int i = 0; i < C; ++i) Mprev[i] = (unsigned)(gg[i] + (int)eTx);
            }
            if ((x >> 4) != gacc) { V2_FLUSH() gacc = x >> 4; }
            V2_ALIGN_ACC(x & 15)
            const int pm1_0 = __builtin_amdgcn_update_dpp(Mleft, (int)Mprev[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);
            const int sxc = min(max(sx, 0), 3);                                      // PW:1503 Score(y, Seq_Bases[x])
            const int rel0 = y0 + lc - a;
            int tg[C];
            int run = PWR_BIG;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int pm1 = i ? (int)Mprev[i > 0 ? i - 1 : 0] : pm1_0;
                const int d = pm1 + ldsS[wave][cs][sxc][lc + i];
                const int u = (int)Mprev[i] + ug[i];
                accC[i] = (accC[i] << 1) | ((d <= u) ? 1u : 0u);
                const int t3 = min(min(d, u), ig[i]);
                tg[i] = ((unsigned)(rel0 + i) < (unsigned)Bx) ? t3 : PWR_BIG;
                run = min(run, tg[i]);
            }
            const int incl = wave_incl_min(run);
            const int excl = __builtin_amdgcn_update_dpp(PWR_BIG, incl, DPP_WAVE_SHR1, 0xF, 0xF, false);
            const int P_end = min(P_in, __builtin_amdgcn_readlane(incl, 63));
            int p = min(P_in, excl);
            if (x != L - 1) {
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    accA[i] = (accA[i] << 1) | ((tg[i] >= p) ? 1u : 0u);
                    p = min(p, tg[i]);
                    Mprev[i] = (rel0 + i < 0) ? PWR_INF : (unsigned)(gg[i] + p);
                }
            } else {
                // last row: PW:1386 "M == M(x,y-1)" also moves left; keep the row for the entry scan
                unsigned Mn[C];
                unsigned fa = 0;
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    fa |= (tg[i] >= p) ? (1u << i) : 0u;
                    p = min(p, tg[i]);
                    Mn[i] = (rel0 + i < 0) ? PWR_INF : (unsigned)(gg[i] + p);
                }
                const unsigned mrow = needP ? ePy : PWR_INF;
                const unsigned left0 = (unsigned)__builtin_amdgcn_update_dpp((int)mrow, (int)Mn[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const unsigned lf = i ? Mn[i > 0 ? i - 1 : 0] : left0;
                    const bool inb = (unsigned)(rel0 + i) < (unsigned)Bx;
                    accA[i] = (accA[i] << 1) | ((((fa >> i) & 1u) || (inb && Mn[i] == lf)) ? 1u : 0u);
                    lastM[wave * MS + lc + i] = inb ? Mn[i] : 0xffffffffu;
                    Mprev[i] = Mn[i];
                }
            }
            nacc = (x & 15) + 1;
            if (lane == 63) {
                ST64(MBP(wave, x), P_end, x + 1);
                ST64(MBM(wave, x), Mprev[C - 1], x + 1);
                if (ms == ms_hi) ST64(PTB(x), P_end, x + 1);
            }
            ran_prev = 1;
            V2_NEXT_ROW()
        }
        if (lane == 0) __hip_atomic_store(&rdone[wave], round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        if (UNI(__hip_atomic_load(&s_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >= NW) break;
    }
    if (round >= max_rounds) {
        if (tid == 0) { m->ok = 0; atomicCAS(&st.hdr->status, 0, PWR_ERR_INTERNAL); }
        return;
    }
    if (tid == 0) {
        m->clk = (unsigned)(__builtin_amdgcn_s_memtime() - t_clk0);
        m->rclk = (unsigned)(__builtin_amdgcn_s_memrealtime() - t_real0);
        m->rounds = round;
        atomicAdd(&st.hdr->cells_computed, m->cells);
    }
#undef MBP
#undef MBM
#undef PTB
#undef LD64
#undef LD32LO
#undef ST64
}

// ---------------------------------------------------------------------------------------------
// fill v3: the same wave pipeline as k_fill_v2, spread over compute units.  Every wave of a DP is its own
// work-group, so each gets a SIMD to itself (in k_fill_v2 the fifth wave of a work-group shares one with the
// first, and that pair sets the pace); the grid is (8, NW, jobs / 8) so that the NW work-groups of one DP land
// on the same XCD and talk through its L2.  What a wave publishes per DP row goes to global memory:
//   gmb[w * gstride + x]  {P_end, tag}   the running minimum its right neighbour continues
// (Ptot, the minimum of the whole row, is the P_end word of the wave that ends the band in that row; and M_last, the
// score N = M - G of the wave's last column, which the right neighbour's first column takes as its left score in the next
// row, is the same number wherever that column lies in the row's band -- DESIGN.md 3.2 --, so it has no word of its own.)
// One aligned 64-bit word, stored and loaded whole (relaxed agent-scope atomics) and self-validating:
// tag = launch epoch << 17 | row + 1, so nothing has to be cleared between launches.  There are no rounds and
// no barriers: a wave simply runs down its rows and waits (bounded by a time-out that flags the job) where a
// word is missing.  Dependencies only point to the left neighbour, whose own never point back, so this cannot
// deadlock as long as all NW work-groups are resident -- NW <= 9 per DP, a few dozen DPs per launch, 256 CUs.
//
// Every work-group has a second wave, the FETCHER.  It sits on another SIMD of the same CU, polls the left
// neighbour's published word of the rows [wx - 1, wx + 63) -- wx = the worker's progress -- and copies every
// valid one into an LDS ring; the worker reads the ring exactly as k_fill_v2 reads its mailboxes (one LDS
// access, waiting in the middle of the row if the word is not there yet).  The worker therefore trails its
// neighbour by one poll of the fetcher (a few DP rows), and the L2 round trip is never on its critical path.
// Ring words keep their row tags, so an old occupant of a slot is never mistaken for the row in demand.
// ---------------------------------------------------------------------------------------------
#ifndef PWR_DIAG_SEG
#define PWR_DIAG_SEG 0              // (-DPWR_DIAG builds: the segment of job 0 whose waves fill the counters and logs; the last one if there are fewer)
#endif
#ifndef PWR_INTERIOR_CLS
#define PWR_INTERIOR_CLS 0          // (4: interior groups run the RIGHT code, experiment on the effect of equal speeds)
#endif
#define V3_TICKS() ((unsigned)(__builtin_amdgcn_s_memtime() >> 10))   // 32-bit time in units of 1024 shader clocks (scalar compares)
#define V3_TIMEOUT_TICKS (1u << 19)                  // about 0.2 s (legitimate waits are microseconds): how long a wave waits for its neighbour before it flags the job
#define V4_RB 128                                    // ring slots (rows); the fetcher looks at most 64 rows ahead

#ifdef PWR_DIAG
#define DG_DECL unsigned long long dg_wait_fast = 0, dg_wait_gen = 0, dg_wait_setup = 0, dg_t = 0, dg_t2 = 0, dg_cyc_int = 0, dg_cyc_gen16 = 0, dg_ts1 = 0, dg_ts2 = 0, dg_tl2 = 0; unsigned dg_log = 0; unsigned dg_int = 0, dg_gen16 = 0, dg_general = 0, dg_nowork = 0, dg_runs = 0, dg_switch = 0;
#define DG_T0() dg_t = __builtin_amdgcn_s_memtime();
#define DG_ADD(ACC) ACC += __builtin_amdgcn_s_memtime() - dg_t;
#define DG_INC(CNT, N) CNT += (N);
#define DG_T2() dg_t2 = __builtin_amdgcn_s_memtime();
#define DG_ADD2(ACC) ACC += __builtin_amdgcn_s_memtime() - dg_t2;
#else
#define DG_T2()
#define DG_ADD2(ACC)
#define DG_DECL
#define DG_T0()
#define DG_ADD(ACC)
#define DG_INC(CNT, N)
#endif
template <int NW, int C, bool WG1>
__global__ __launch_bounds__(WG1 ? NW * 64 : 128) void k_fill_v3(DState st, JobBufs jb)
{
    constexpr int MS = 64 * C, RS = NW * MS;
    // WG1: the NW waves of a segment are ONE work-group (no fetchers): a wave stores the words it publishes straight into its
    // right neighbour's ring in LDS (and the running minimum also to global memory, where the rare readers of a row's total
    // minimum find it).  A hand-over is then an LDS round trip instead of an L2 one plus the fetcher's poll; a ring slot is
    // written again only when the reader is past it (its progress counter), so no wave runs more than RB rows ahead of its
    // reader.  On its own CU a segment has every SIMD to two of its waves (NW = 8).
    constexpr int NL = WG1 ? NW : 1;                                      // waves whose tables and rings live in this work-group's LDS
    constexpr int RB = WG1 ? 64 : V4_RB;                                  // ring slots (rows)
    __shared__ __attribute__((aligned(16))) int ldsS1[NL][2][4][MS];
    __shared__ unsigned long long rP[NL][RB];                            // the left neighbour's {P_end, tag}
    __shared__ int wprog[NL], wdone;                                     // worker's progress (rows), worker finished
    // virtual job = (job, segment): segment s of job j is slot j * smax + s, so the segments of a job spread over the XCDs
    const int vjob = WG1 ? (int)blockIdx.x : (int)(blockIdx.x + 8 * blockIdx.z), lane = threadIdx.x & 63;
    const int role = WG1 ? 0 : UNI((int)threadIdx.x >> 6);               // 0 worker, 1 fetcher
    const int wave = WG1 ? UNI((int)threadIdx.x >> 6) : (int)blockIdx.y;
    const int lw = WG1 ? wave : 0, wr = WG1 ? (wave + 1) % NW : 0;       // this wave's LDS slot, its right neighbour's
    if (vjob >= jb.njobs_launched * jb.smax) return;
    const int job = vjob / jb.smax;
    const SegDesc *const sd = jb.seg + (size_t)job * SEG_MAX + (vjob % jb.smax);
    JobMeta *m = &jb.meta[job];
    if (st.hdr->fallback > 0 && jb.v2_follows) return;                            // k_fill_v2 stands in (after a stall)
    if (!m->active || m->L <= 0 || !m->ok || m->wide || !sd->active || NOT_MINE(jb, job)) return;
    // The segment is a DP of its own on the rows [xb, xe) of the job: x below counts from xb, and everything indexed by DP
    // row is addressed from there.  Its first row starts free (PW:265) whether it is the row's first base or not; its last
    // row is the DP's last row (PW:1386, entry scan) only in the job's last segment.
    const int seg_xb = UNI(sd->xb), seg_fin = UNI(sd->fin);
    const int L = UNI(sd->xe) - seg_xb;
    const int Lf = seg_fin ? L - 1 : L;                                           // rows below Lf are ordinary rows
    const int x_own = UNI(sd->xown) - seg_xb;                                     // rows below it are the warm-up: nothing of them is kept
    const int g_own = x_own >> 4;
    const int chkA = x_own > 0 ? x_own : -1, chkB = seg_fin ? -1 : L;            // after these rows' predecessors the scores are left for the check
    unsigned *const chk_w = jb.chk + (((size_t)job * (SEG_MAX + 1) + sd->s) * 2 + 0) * (size_t)jb.NC;       // [s][0]: this segment after its warm-up
    unsigned *const chk_t = jb.chk + (((size_t)job * (SEG_MAX + 1) + sd->s + 1) * 2 + 1) * (size_t)jb.NC;   // [s + 1][1]: what the next one must match
    const unsigned long long t_clk0 = __builtin_amdgcn_s_memtime(), t_real0 = __builtin_amdgcn_s_memrealtime();
    for (int i = threadIdx.x; i < NL * RB; i += blockDim.x) (&rP[0][0])[i] = 0;   // (another work-group's words of this launch may lie here)
    if (threadIdx.x < NL) wprog[threadIdx.x] = 0;
    if (threadIdx.x == 0) wdone = 0;
    __syncthreads();

    const int wl = (wave + NW - 1) % NW;
    const unsigned tagbase = jb.tagbase;
    const size_t gstride = (size_t)jb.gstride;
    unsigned long long *const gmy = jb.gmb + ((size_t)job * NW + wave) * gstride + (size_t)sd->grow0;
    const unsigned long long *const gleftw = jb.gmb + ((size_t)job * NW + wl) * gstride + (size_t)sd->grow0;
    // Ptot(r), the minimum of the whole DP row r (the virtual extension of PW:285-295 is G + Ptot): it is the P_end word of
    // the wave that holds the band's last macro-strip in row r -- read straight from there, on the rare occasions it is needed
    const unsigned long long *const gjob = jb.gmb + (size_t)job * NW * gstride + (size_t)sd->grow0;
#define PTOT_PTR(AP, BP, R) (gjob + ((size_t)((((AP) + (BP) - 1 - lo) / MS) % NW)) * gstride + (size_t)(R))
    int *const abortf = &m->abort;
#define GLD(PTR) __hip_atomic_load((PTR), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define GST(PTR, VAL, ROW) __hip_atomic_store((PTR), ((unsigned long long)(tagbase | (unsigned)((ROW) + 1)) << 32) | (unsigned)(VAL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define GST2(PTR, VAL, TAG) __hip_atomic_store((PTR), ((unsigned long long)(TAG) << 32) | (unsigned)(VAL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define TAGOF(W64) ((unsigned)((W64) >> 32))
#define LLD(REF) __hip_atomic_load(&(REF), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LST(REF, V) __hip_atomic_store(&(REF), (V), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

    if (!WG1 && role == 1) {
        // ---- fetcher
        // One poll = one L2 round trip (the abort flag is looked at every 16th poll, in the same batch of loads); the lag of
        // a worker behind its neighbour is this loop's period, and it is paid NW - 1 times per lap of the ring of waves.
        for (unsigned it = 0;; ++it) {
            if (UNI(LLD(wdone))) break;
            const int wx = UNI(LLD(wprog[lw]));
            const int r = wx - 1 + lane;                                          // row wx needs the word of row wx - 1 too
            const bool inr = r >= 0 && r < L;
            unsigned long long p = 0;
            int ab = 0;
            if (inr) p = GLD(gleftw + (size_t)r);
            if ((it & 15u) == 15u) ab = GLD(abortf);
            if (inr && TAGOF(p) == (tagbase | (unsigned)(r + 1))) LST(rP[lw][r & (RB - 1)], p);   // (the word vouches for itself)
            // (no time-out of its own: the worker has one, and its end -- wdone -- or the job's abort flag end this loop)
            if (UNI(ab)) break;
        }
        return;
    }

    // ---- worker
    const int lo = UNI(m->lo), hi = UNI(m->hi), W = UNI(m->W), B = st.B, H = st.H;
    const int *way = jb.way + (size_t)job * jb.Lmax + seg_xb;
    const uint8_t *seq = st.seq + st.rowoff[UNI(m->k)] + seg_xb;
    const int4 *rec2 = jb.rec2 + (size_t)job * jb.colcap * 2;
    uint32_t *dirs = jb.dirs + (size_t)job * jb.dirstride + (size_t)(seg_xb >> 4) * RS;
    unsigned *lastM = jb.lastM + (size_t)job * jb.NC;
    const int lc = lane * C;
    // The row is carried as N(x,y) = M(x,y) - G(y): a strip's constants are turned once, here, into what a
    // cell adds to N -- S_b(y) - G(y) + G(y-1) for the diagonal (G(y-1): the lane's column before, the left lane's last one,
    // GL for the strip's first column), up(y) for the column itself; INF - G(y) is "unreachable" as N.  The columns past hi
    // keep their sentinels as they are: nothing is added to them, so nothing wraps.
#define V4_LOADS(MSX, SLOT, AU, AG, AI, GL)                                                      \
    {                                                                                            \
        const int yq_ = lo + (MSX) * MS - 1;                                                     \
        GL = (yq_ >= lo && yq_ <= hi) ? UNI(rec2[2 * (yq_ - lo) + 1].y) : 0;                     \
        int4 p_[C];                                                                              \
        _Pragma("unroll") for (int i = 0; i < C; ++i) {                                          \
            const int y_ = lo + (MSX) * MS + lc + i;                                             \
            p_[i] = make_int4(PWR_BIG / 2, PWR_BIG / 2, PWR_BIG / 2, PWR_BIG / 2);               \
            int4 q_ = make_int4(PWR_BIG / 2, 0, PWR_BIG / 2, 0);                                 \
            if (y_ <= hi) { p_[i] = rec2[2 * (y_ - lo)]; q_ = rec2[2 * (y_ - lo) + 1]; }         \
            AU[i] = q_.x + q_.y; AG[i] = q_.y; AI[i] = q_.z;                                     \
        }                                                                                        \
        const int gl0_ = __builtin_amdgcn_update_dpp(GL, AG[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);   \
        _Pragma("unroll") for (int i = 0; i < C; ++i) {                                          \
            const int y_ = lo + (MSX) * MS + lc + i;                                             \
            const int gp_ = y_ <= hi ? (i ? AG[i > 0 ? i - 1 : 0] : gl0_) : 0;                   \
            ldsS1[lw][SLOT][0][lc + i] = p_[i].x + gp_; ldsS1[lw][SLOT][1][lc + i] = p_[i].y + gp_;      \
            ldsS1[lw][SLOT][2][lc + i] = p_[i].z + gp_; ldsS1[lw][SLOT][3][lc + i] = p_[i].w + gp_;      \
        }                                                                                        \
    }

    int ug[C], gg[C], ig[C];
    int nu[C], ng[C], ni[C];
    int gleft = 0, gleftn = 0;
    // the wave's first macro-strip: the first one of its residue class that is not left of the first row's band
    const int ms_first = (max(0, UNI(way[0]) - H) - lo) / MS;
    int ms = ms_first + (((wave - ms_first) % NW) + NW) % NW, msn = ms + NW;
    int cs = 0;
    V4_LOADS(ms, 0, ug, gg, ig, gleft)
    V4_LOADS(msn, 1, nu, ng, ni, gleftn)

    // Where a warm-up starts.  Any row vector will do for "the scores above the segment's first row" -- whether the warm-up
    // forgot it is checked (k_seg_check) --, but how soon it is forgotten depends on it.  The free start of PW:265 (every
    // column 0) lets paths begin anywhere in the band for nothing, and they have to die out or leave the band before the rows
    // are parallel to the true ones (about 1.5 bandwidths of band movement).  The true vector is a steep V around the cell
    // the best path goes through, and the row's present placement is the best guess at that cell: so the warm-up starts from
    // ONE cell, the column of the base before its first row (score 0, every other column unreachable) -- the cells right of
    // it get their scores from the row's own scan, the cells left of it stay unreachable until the band has left them behind,
    // which takes half a bandwidth (measured with the oracle's tallies: scripts/dev/start_vectors.py).  Not when that
    // column lies left of the first row's band (a run of blanks in the row): then the free start it is.
    const int src_prev = (seg_xb > 0 && jb.src_start) ? UNI(way[-1]) : -1;
    const int src_c = src_prev >= max(0, UNI(way[0]) - H) ? src_prev : -1;
    unsigned Mprev[C], accA[C], accC[C];                                          // Mprev holds N = M - G: score 0 is -G, unreachable INF - G
#pragma unroll
    for (int i = 0; i < C; ++i) { Mprev[i] = (unsigned)((src_c < 0 || lo + ms * MS + lc + i == src_c) ? -gg[i] : ig[i]); accA[i] = accC[i] = 0; }
    int gacc = -1, nacc = 0;
    int ran_prev = 0;
    int x = 0, blk = 0;
    int wcur = way[min(lane, L - 1)], scur = seq[min(lane, L - 1)];
    int wnxt = way[min(64 + lane, L - 1)], snxt = seq[min(64 + lane, L - 1)];
    const uint4 *desc = jb.desc + (size_t)job * jb.Lmax + seg_xb;
    const int fsh = 4 * (wave & 7);
    const unsigned *descw = (const unsigned *)desc + 1 + (wave >> 3);      // this wave's flag word of a descriptor
    unsigned dca = desc[min(lane, L - 1)].x, dcf = descw[4 * min(lane, L - 1)] >> fsh;
    unsigned dna = desc[min(64 + lane, L - 1)].x, dnf = descw[4 * min(64 + lane, L - 1)];      // (shifted when the block becomes current)
    int a = max(0, __builtin_amdgcn_readlane(wcur, 0) - H), a_prev = 0, Bx_prev = 0;
    int sx = __builtin_amdgcn_readlane(scur, 0);

    // the scores of the row just done, for k_seg_check: band cells of this wave's macro-strip, indexed like lastM
#define V4_CHK_STORE(XNEXT, AF, BEND)                                                            \
    if ((XNEXT) == chkA || (XNEXT) == chkB) {                                                    \
        unsigned *cv_ = (XNEXT) == chkA ? chk_w : chk_t;                                         \
        _Pragma("unroll") for (int i = 0; i < C; ++i) {                                          \
            const int y_ = lo + ms * MS + lc + i;                                                \
            cv_[wave * MS + lc + i] = (y_ >= (AF) && y_ < (BEND)) ? (unsigned)gg[i] + Mprev[i] : 0xffffffffu;   /* true scores: G + N */ \
        }                                                                                        \
    }
#define V4_ALIGN_ACC(WANT)                                                                       \
    if (nacc != (WANT)) {                                                                        \
        const int sh_ = (WANT) - nacc;                                                           \
        _Pragma("unroll") for (int i = 0; i < C; ++i) { accA[i] <<= sh_; accC[i] <<= sh_; }      \
        nacc = (WANT);                                                                           \
    }
#define V4_FLUSH()                                                                               \
    if (gacc >= 0) {                                                                             \
        V4_ALIGN_ACC(16)                                                                         \
        uint32_t *d_ = dirs + (size_t)gacc * RS + (size_t)wave * MS + (size_t)lc;                \
        _Pragma("unroll") for (int i = 0; i < C; ++i) { if (gacc >= g_own) d_[i] = accA[i] | (accC[i] << 16); accA[i] = accC[i] = 0; } \
        gacc = -1; nacc = 0;                                                                     \
    }
#define V4_ROTATE_BLOCK()                                                                        \
    {                                                                                            \
        blk = x >> 6;                                                                            \
        wcur = wnxt; scur = snxt; dca = dna; dcf = dnf >> fsh;     \
        wnxt = way[min(x + 64 + lane, L - 1)];                                                   \
        snxt = seq[min(x + 64 + lane, L - 1)];                                                   \
        dna = desc[min(x + 64 + lane, L - 1)].x; dnf = descw[4 * min(x + 64 + lane, L - 1)];     \
    }
#define V4_NEXT_ROW()                                                                            \
    {                                                                                            \
        a_prev = a; Bx_prev = Bx;                                                                \
        ++x;                                                                                     \
        if (lane == 0) LST(wprog[lw], x);                                                            \
        if (x < L) {                                                                             \
            if ((x >> 6) != blk) V4_ROTATE_BLOCK()                                               \
            a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);                             \
            sx = __builtin_amdgcn_readlane(scur, x & 63);                                        \
        }                                                                                        \
    }

    DG_DECL
#ifdef PWR_DIAG
    const bool dg_me = sd->s == min(PWR_DIAG_SEG, UNI(m->nseg) - 1);             // the per-wave counters and logs are one segment's (the time line below is every segment's)
    unsigned long long *const tl = jb.diag + ((size_t)job * 32 + 31) * 4096 + (size_t)(sd->s * NW + wave) * 6;   // the segment's time line
    if (lane == 0 && sd->s * NW + wave < 680) { tl[0] = t_real0; tl[1] = __builtin_amdgcn_s_memrealtime(); tl[2] = 0; }
#endif
    // A wave takes its next macro-strip over at the 16-row boundary BEFORE the strip's first row with work: in the rows in
    // between every cell of the strip lies past the band's end and is masked by the right-hand guard, which leaves exactly the
    // virtual extension G + Ptot in Mprev (PW:285-295) -- but the strip starts with a whole group of straight-line rows, not
    // with a stub of rows in the slow one-row loop, right where the pipeline's critical path runs.  The gather's flags do not
    // know these rows (nor that the strip's first row with work now has a row above it): they are overridden here.
#define V4_EARLY_MASKS()                                                                         \
    if (early_hi >= (blk << 6)) {                                                                \
        const int b0_ = blk << 6;                                                                \
        const int lo_ = max(early_lo, b0_) - b0_, hi_ = min(early_hi, b0_ + 64) - b0_;           \
        const unsigned long long me_ = hi_ > lo_ ? ((hi_ - lo_ >= 64 ? ~0ull : ((1ull << (hi_ - lo_)) - 1ull)) << lo_) : 0ull; \
        const unsigned long long mf_ = early_hi < b0_ + 64 ? 1ull << (early_hi - b0_) : 0ull;    \
        bOm |= me_ | mf_; bMm |= me_ | mf_; bPm |= me_; bTm |= me_;                              \
    }
    bool dead = jb.stall_test && vjob == 0 && wave == 0;                          // (test hook: as if the neighbour never answered)
    int first_pending = 0;                                                       // row x is the wave's first on its macro-strip: the fast path takes it
    int early_lo = 0, early_hi = -1;                                             // rows [early_lo, early_hi) run ahead of the strip's first row with work, early_hi
    while (x < L && !dead) {
        ran_prev = UNI(ran_prev); gacc = UNI(gacc); nacc = UNI(nacc); blk = UNI(blk); ms = UNI(ms); cs = UNI(cs); gleft = UNI(gleft);
        x = UNI(x);
#ifdef PWR_DIAG
        if (ran_prev && !dg_tl2) { dg_tl2 = __builtin_amdgcn_s_memrealtime(); if (lane == 0 && sd->s * NW + wave < 680) { tl[2] = dg_tl2; tl[5] = (unsigned long long)x; } }
#endif
        // ---- fast path: a RUN of ordinary rows (flagged by the gather), from x to the first row that is not ordinary.
        // What a row needs beyond its cells is reduced to the hand-over: the left neighbour's self-validating words are
        // taken from the ring before the scan and checked after it, where the wave waits if they are not there yet -- so it
        // trails its neighbour by a few rows only.  Rows are processed in their 16-row groups (one 32-bit word of traceback
        // bits per column and group); a complete group whose rows all play the same role runs as straight-line code:
        //   INTERIOR  the macro-strip lies inside the band, it is neither the band's first nor its last: no band guards;
        //   RIGHT     the band ends in the macro-strip: guard y < band end, the row minimum Ptot is posted as well;
        //   LEFT      the band starts in the macro-strip: guard y >= anf, nothing is needed from the neighbour;
        // anything else (a change of role inside the group, a partial group) takes the same code with run-time flags.
        // All roles must cost about the same: a wave that is slower than its neighbour while it is the band's last strip
        // falls behind for good, and every row of lag per hop is paid NW - 1 times per lap of the ring (measured).
        if ((ran_prev || first_pending) && x < Lf) {
            unsigned long long bOm = __builtin_amdgcn_ballot_w64((dcf & 1u) != 0);
            const bool first = UNI(first_pending) != 0;
            if (first || ((bOm >> (x & 63)) & 1ull)) {
                first_pending = 0;
                unsigned long long bPm = __builtin_amdgcn_ballot_w64((dcf & 2u) != 0);       // needs the neighbour's running minimum
                unsigned long long bMm = __builtin_amdgcn_ballot_w64((dcf & 4u) != 0);       // left score = neighbour's M_last(x-1)
                unsigned long long bTm = __builtin_amdgcn_ballot_w64((dcf & 8u) != 0);       // the band ends here: guard against columns past it
                if (first) { bOm |= 1ull << (x & 63); bMm |= 1ull << (x & 63); }             // (its left score is worked out below)
                V4_EARLY_MASKS()
                // per row of the 64-block, one lane each: anf, band end, byte offset of the row's base in the LDS table
                int dcaf = (int)(dca & 0xffffffu), dcb = min(dcaf + B, W);
                unsigned dcs = min(dca >> 24, 3u) * (unsigned)(MS * 4);
                if ((x >> 4) != gacc) { V4_FLUSH() gacc = x >> 4; }
                V4_ALIGN_ACC(x & 15)
                if (lane == 0) LST(wprog[lw], x);                                    // the fetcher looks at the rows [x - 1, x + 63)
                unsigned mlast_v = 0;                                            // M_last(x-1) of the left neighbour
                if (first) {
                    // The wave's first row on this macro-strip (it has just taken it over, or the band has just reached it).
                    // This is where the pipeline's critical path runs -- the band's last strip can only start when its left
                    // neighbour delivers, and the next one waits for it in turn --, so everything that does not need the
                    // neighbour's word of row x is done here, before it: the scores the rows above left behind are the
                    // virtual extension G + Ptot(x-1) (PW:285-295), and the score left of the strip is the neighbour's
                    // M_last(x-1), or that extension, or INF (PW:276).  Row x itself then runs like any other row and waits for
                    // P_end(x) only after its scan.
                    const unsigned tagp = tagbase | (unsigned)x;
                    const int yq = lo + ms * MS - 1;
                    const bool needM = yq >= a_prev && yq < a_prev + Bx_prev;
                    unsigned long long eT = 0, eM = 0;
                    DG_T0()
#ifdef PWR_DIAG
                    const unsigned long long ev_t0 = __builtin_amdgcn_s_memrealtime();
#endif
                    const unsigned t0 = V3_TICKS();
                    for (unsigned spin = 1;; ++spin) {
                        eT = GLD(PTOT_PTR(a_prev, Bx_prev, x - 1));
                        eM = LLD(rP[lw][(x - 1) & (RB - 1)]);                        // (M_last(x-1) = P_end(x-1) where needM)
                        if (UNI(TAGOF(eT)) == tagp && (!needM || UNI(TAGOF(eM)) == tagp)) break;
                        if ((spin & 1023u) == 0 && (V3_TICKS() - t0 > V3_TIMEOUT_TICKS || UNI(GLD(abortf)))) { dead = true; break; }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    DG_ADD(dg_wait_gen)
#ifdef PWR_DIAG
                    if (lane == 0 && dg_me && dg_general < 36) {
                        unsigned long long *ev = jb.diag + ((size_t)job * 32 + wave) * 4096 + 16 + 3 * dg_general;
                        ev[0] = (unsigned long long)x; ev[1] = ev_t0; ev[2] = __builtin_amdgcn_s_memrealtime();
                    }
#endif
                    DG_INC(dg_general, 1)
                    if (dead) break;
                    const int eTx = (int)UNI((unsigned)eT);
#pragma unroll
                    for (int i = 0; i < C; ++i) Mprev[i] = (unsigned)eTx;          // N of the extension G + Ptot
                    mlast_v = yq < a_prev ? PWR_INF - (unsigned)gleft : (needM ? UNI((unsigned)eM) : (unsigned)eTx);
                    ran_prev = 1;
                } else if ((bMm >> (x & 63)) & 1ull) {
                    const unsigned tagp = tagbase | (unsigned)x;
                    unsigned long long w_ = LLD(rP[lw][(x - 1) & (RB - 1)]);
                    if (UNI(TAGOF(w_)) != tagp) {                                   // (bounded by a time-out that flags the job)
                        DG_T0()
                        const unsigned t0 = V3_TICKS();
                        for (unsigned spin = 1;; ++spin) {
                            w_ = LLD(rP[lw][(x - 1) & (RB - 1)]);
                            if (UNI(TAGOF(w_)) == tagp) break;
                            if ((spin & 1023u) == 0 && (V3_TICKS() - t0 > V3_TIMEOUT_TICKS || UNI(GLD(abortf)))) { dead = true; break; }
                            __builtin_amdgcn_s_sleep(1);
                        }
                        DG_ADD(dg_wait_setup)
                        if (dead) break;
                    }
                    mlast_v = (unsigned)w_;
                }
                int ycol[C];                                                     // absolute columns of this lane's cells
#pragma unroll
                for (int i = 0; i < C; ++i) ycol[i] = lo + ms * MS + lc + i;
                const char *const stab = (const char *)&ldsS1[lw][cs][0][lc];          // + dcs: the row's substitution scores S_b - G
                int sgr[C];
                {
                    const int *const srow0 = (const int *)(stab + __builtin_amdgcn_readlane((int)dcs, x & 63));
#pragma unroll
                    for (int i = 0; i < C; ++i) sgr[i] = srow0[i];
                }
                int af_done = a_prev;
                int g_af = 0, g_be = 0, g_cs = 0, g_cp = -1;                      // (see below: the current group's rows, lane = row of the group)
                DG_INC(dg_runs, 1)
                while (true) {
                    const int r_beg = x & 15, g0 = x - r_beg, r0 = g0 & 63;
                    int nrun = __builtin_ctz(~((unsigned)(bOm >> (r0 + r_beg)) & 0xffffu) | (1u << (16 - r_beg)));   // ordinary rows from x on, within the group
                    nrun = min(nrun, Lf - x);
                    if (nrun <= 0) break;
                    const unsigned nPm = (unsigned)(bPm >> r0) & 0xffffu, kMm = (unsigned)(bMm >> r0) & 0xffffu, eTm = (unsigned)(bTm >> r0) & 0xffffu;
                    // the rows from x on that play the same role as row x: one stretch
                    const unsigned p0 = (nPm >> r_beg) & 1u, m0 = (kMm >> r_beg) & 1u, t0_ = (eTm >> r_beg) & 1u;
                    // (whether the band ends in the strip -- Ptot is posted -- does not split a stretch of neighbour-fed rows: the row
                    // where the next strip's wave takes over is exactly where this wave must not dawdle)
                    const unsigned diff = ((nPm ^ (0u - p0)) | (kMm ^ (0u - m0)) | ((p0 & m0) ? 0u : (eTm ^ (0u - t0_)))) & 0xffffu;
                    const int nsame = __builtin_ctz((diff >> r_beg) | 0x10000u);
                    // (a WHOLE group whose rows change role on the way is not cut into stretches either: it runs as straight-line
                    // code with the roles as per-row flags -- the stubs of the one-row loop were where every wave in turn held
                    // the whole pipeline up)
                    const bool mixed16 = r_beg == 0 && nrun == 16 && nsame < 16;
                    const int r_e = mixed16 ? 16 : r_beg + min(nrun, nsame);
                    const unsigned et_here = (eTm >> r_beg) & ((1u << (r_e - r_beg)) - 1u);
                    const int cls = mixed16 ? 3 : ((p0 & m0) ? (et_here ? 1 : 0) : ((p0 | m0 | t0_) == 0u ? 2 : 3));
                    if (gacc < 0) gacc = x >> 4;
#ifdef PWR_DIAG
                    if (!dg_ts1 && x >= 1024) dg_ts1 = __builtin_amdgcn_s_memrealtime();
                    if (!dg_ts2 && x >= 2048) dg_ts2 = __builtin_amdgcn_s_memrealtime();
#endif
                    if (WG1) {
                        // the ring slots of this group's rows hold the rows RB earlier: is the right neighbour past them?
                        const int need = g0 + 16 - RB + 2;
                        if (need > 0 && UNI(LLD(wprog[wr])) < need) {
                            DG_T0()
                            const unsigned t0 = V3_TICKS();
                            for (unsigned spin = 1;; ++spin) {
                                if (UNI(LLD(wprog[wr])) >= need) break;
                                if ((spin & 1023u) == 0 && (V3_TICKS() - t0 > V3_TIMEOUT_TICKS || UNI(GLD(abortf)))) { dead = true; break; }
                                __builtin_amdgcn_s_sleep(1);
                            }
                            DG_ADD(dg_wait_setup)
                            if (dead) break;
                        }
                    }
                    unsigned long long *const gq0 = gmy + (size_t)g0;
                    const unsigned tag_g0 = tagbase | (unsigned)g0;                 // (the rows' tags are this + r + 1)
                    const unsigned long long *const ringP = &rP[lw][g0 & (RB - 1)];   // the group's 16 consecutive slots
                    // the group's rows in lanes 0..16 of their own registers (lane r: row g0 + r; lane 16: the first row of the next
                    // group, for the look-ahead of the substitution column): every v_readlane below then has a constant lane
                    if (g0 != g_cp) {
                        const int src = 4 * min(r0 + lane, 63);
                        g_af = __builtin_amdgcn_ds_bpermute(src, dcaf);
                        g_be = __builtin_amdgcn_ds_bpermute(src, dcb);
                        g_cs = __builtin_amdgcn_ds_bpermute(src, (int)dcs);
                        g_cp = g0;
                    }
                    // The scan is six v_min_i32_dpp, each reading the register the one before it wrote: a DPP operand needs two wait
                    // states behind the VALU write, and where nothing stands between two steps the compiler pads with an s_nop --
                    // which takes a lone wave's issue slot like any instruction.  So the row's own work that does not depend on the
                    // scan is dealt out over the six gaps, two instructions or more each, pinned by scheduling fences: the ring
                    // read, the next row's substitution scores (address, then the reads), the tag, the C bits of a row with record
                    // (d and u stay live for them; a v_cmp and the v_addc that takes its mask stand a scan step apart, the same two
                    // wait states), and the band guard of the NEXT row -- its compares depend on the descriptor alone, so their masks
                    // are made a row ahead and wait in scalar registers (gd[]; guard_head makes them for a stretch's first row).
                    // Pure scheduling: every register holds what it held.
                    unsigned long long gd[C];
#pragma unroll
                    for (int i = 0; i < C; ++i) gd[i] = ~0ull;
                    auto guard_head = [&](const int r, auto cls_) __attribute__((always_inline)) {
                        constexpr int CLS = decltype(cls_)::value;
                        if (CLS == 1 || CLS == 2 || CLS == 4) {
                            const int e_ = __builtin_amdgcn_readlane(CLS == 2 ? g_af : g_be, r);
#pragma unroll
                            for (int i = 0; i < C; ++i) gd[i] = __builtin_amdgcn_sicmp(ycol[i], e_, CLS == 2 ? ICMP_SGE : ICMP_SLT);
                        }
                    };
                    auto group_row = [&](const int r, auto cls_, auto bits_) __attribute__((always_inline)) {
                        constexpr int CLS = decltype(cls_)::value;                 // 0 INTERIOR, 1 RIGHT, 2 LEFT, 3 run-time flags
                        constexpr bool BITS = decltype(bits_)::value;              // false: a row of the warm-up, whose record nobody keeps
                        constexpr bool AHEAD = CLS == 1 || CLS == 2 || CLS == 4;   // one guard, its masks made a row ahead (gd)
                        constexpr int CH = (C + 1) / 2;                            // the cells' fillers come in two halves: [0, CH) and [CH, C)
                        bool bP = CLS <= 1 || CLS == 4, bM = CLS <= 1 || CLS == 4;
                        if (CLS == 3) { bP = (nPm >> r) & 1u; bM = (kMm >> r) & 1u; }
                        int af = 0, bend = 0;
                        if (CLS == 3) { af = __builtin_amdgcn_readlane(g_af, r); bend = __builtin_amdgcn_readlane(g_be, r); }
                        const int Mleft_v = bM ? (int)mlast_v : (int)PWR_INF - gleft;
                        const int pm1_0 = __builtin_amdgcn_update_dpp(Mleft_v, (int)Mprev[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);
                        int tg[C], dq[C], uq[C];
                        int run = FBIG;
#pragma unroll
                        for (int i = 0; i < C; ++i) {
                            const int pm1 = i ? (int)Mprev[i > 0 ? i - 1 : 0] : pm1_0;
                            const int d = pm1 + sgr[i];
                            const int u = (int)Mprev[i] + ug[i];
                            dq[i] = d; uq[i] = u;
                            const int t3 = min(min(d, u), ig[i]);
                            bool inb = true;
                            if (AHEAD) inb = __builtin_amdgcn_inverse_ballot_w64(gd[i]);
                            if (CLS == 3) inb = (unsigned)(ycol[i] - af) < (unsigned)(bend - af);
                            tg[i] = inb ? t3 : FBIG;
                            run = min(run, tg[i]);
                        }
                        unsigned long long fP = 0, cm[C];
                        unsigned tagx = 0;
                        int gb = 0, soff = 0;
                        const int *srow = nullptr;
#define V4_SCAN_STEP(CTRL, RMASK) { const int t_ = __builtin_amdgcn_update_dpp(PWR_BIG, incl, CTRL, RMASK, 0xF, false); incl = min(incl, t_); }
#define V4_FENCE() __builtin_amdgcn_sched_barrier(0)
                        // the fillers, each pinned where it stands; a VALU that reads a scalar register stands two instructions behind
                        // the VALU that wrote it (v_readlane -> address, v_cmp -> v_addc / v_cndmask), and two v_addc are not neighbours
#define V4_F_RING() { fP = LLD(ringP[r]); V4_FENCE(); }                                           /* the neighbour's word of this row: value and tag in one 64-bit read */
#define V4_F_SOFF() { soff = __builtin_amdgcn_readlane(g_cs, r + 1); V4_FENCE(); }                /* (past the block's end: reloaded below) */
#define V4_F_EDGE() { if (AHEAD) { gb = __builtin_amdgcn_readlane(CLS == 2 ? g_af : g_be, r + 1); V4_FENCE(); } }
#define V4_F_TAG()  { tagx = tag_g0 + (unsigned)(r + 1); if (CLS == 2) asm volatile("" :: "s"(tagx)); V4_FENCE(); }   /* (LEFT: only the store wants it, and the compiler would move it there) */                            /* = tagbase | (xr + 1): g0 is a multiple of 16 */
#define V4_F_SROW() { srow = (const int *)(stab + soff); V4_FENCE(); }
#define V4_F_SGR(LO, HI) { _Pragma("unroll") for (int i = 0; i < C; ++i) if (i >= (LO) && i < (HI)) sgr[i] = srow[i]; V4_FENCE(); }
#define V4_F_CC(I)  { if ((I) < C) { cm[(I) < C ? (I) : 0] = __builtin_amdgcn_sicmp(dq[(I) < C ? (I) : 0], uq[(I) < C ? (I) : 0], ICMP_SLE); V4_FENCE(); } }
#define V4_F_CP(I)  { if ((I) < C) { accC[(I) < C ? (I) : 0] = acc_push(accC[(I) < C ? (I) : 0], cm[(I) < C ? (I) : 0]); V4_FENCE(); } }
#define V4_F_GD(I)  { if (AHEAD && (I) < C) { gd[(I) < C ? (I) : 0] = __builtin_amdgcn_sicmp(ycol[(I) < C ? (I) : 0], gb, CLS == 2 ? ICMP_SGE : ICMP_SLT); V4_FENCE(); } }
#define V4_F_BIG()  { asm volatile("" : "+v"(big)); V4_FENCE(); }                                  /* the last step's neutral element, in its register two instructions ahead of the step */
                        int big = PWR_BIG;
                        auto gap = [&](auto k_) __attribute__((always_inline)) {
                            constexpr int K = decltype(k_)::value + (CLS == 2 ? 1 : 0);   // (LEFT reads no ring: its list starts with the second gap's)
                            if constexpr (decltype(k_)::value == 5 && CLS != 2) V4_F_BIG()   // (LEFT has no branch behind the scan: its last step is one v_min_i32_dpp as it stands)
                            if constexpr (K == 0) V4_F_RING()
                            if constexpr (!BITS && AHEAD) {
                                if constexpr (K == 1) { V4_F_SOFF() V4_F_EDGE() }
                                if constexpr (K == 2) { V4_F_SROW() V4_F_TAG() }
                                if constexpr (K == 3) { V4_F_SGR(0, CH) V4_F_SGR(CH, C) }
                                if constexpr (K == 4) { _Pragma("unroll") for (int i = 0; i < CH; ++i) V4_F_GD(i) }
                                if constexpr (K == 5) { _Pragma("unroll") for (int i = CH; i < C; ++i) V4_F_GD(i) }
                            }
                            if constexpr (!BITS && !AHEAD) {
                                if constexpr (K == 1) { V4_F_SOFF() V4_F_TAG() }
                                if constexpr (K == 2) { V4_F_SROW() V4_F_SGR(0, CH) }
                                if constexpr (K == 3) { V4_F_SGR(CH, C) }
                            }
                            if constexpr (BITS) {
                                // (the instruction behind a v_addc is never a compare: the compiler takes an inline asm's results for
                                // hazardous to whatever touches their registers next, and a compare likes the carry's scalar pair)
                                if constexpr (K == 1) { V4_F_SOFF() V4_F_EDGE() }
                                if constexpr (K == 2) { V4_F_SROW() V4_F_SGR(0, CH) }
                                if constexpr (K == 3) { _Pragma("unroll") for (int i = 0; i < C - 1; ++i) V4_F_CC(i) }
                                if constexpr (K == 4) { V4_F_CC(C - 1) _Pragma("unroll") for (int i = 0; i < CH; ++i) { V4_F_CP(i) if (i == 0) V4_F_SGR(CH, C) } }
                                if constexpr (K == 5) { _Pragma("unroll") for (int i = CH; i < C; ++i) { V4_F_CP(i) if (i == CH) { V4_F_TAG() V4_F_GD(0) } } if (CH == C) { V4_F_TAG() V4_F_GD(0) } }
                                if constexpr (K == 6) { _Pragma("unroll") for (int i = 1; i < CH; ++i) V4_F_GD(i) }
                                if constexpr (K == 7) { _Pragma("unroll") for (int i = CH; i < C; ++i) V4_F_GD(i) }
                            }
                        };
                        using std::integral_constant;
                        int incl = run;
                        V4_FENCE(); gap(integral_constant<int, 0>{}); V4_SCAN_STEP(DPP_ROW_SHR(1), 0xF) V4_FENCE();
                        gap(integral_constant<int, 1>{}); V4_SCAN_STEP(DPP_ROW_SHR(2), 0xF) V4_FENCE();
                        gap(integral_constant<int, 2>{}); V4_SCAN_STEP(DPP_ROW_SHR(4), 0xF) V4_FENCE();
                        gap(integral_constant<int, 3>{}); V4_SCAN_STEP(DPP_ROW_SHR(8), 0xF) V4_FENCE();
                        gap(integral_constant<int, 4>{}); V4_SCAN_STEP(DPP_ROW_BCAST15, 0xA) V4_FENCE();
                        gap(integral_constant<int, 5>{});
                        { const int t_ = __builtin_amdgcn_update_dpp(big, incl, DPP_ROW_BCAST31, 0xC, 0xF, false); incl = min(incl, t_); } V4_FENCE();
                        gap(integral_constant<int, 6>{}); gap(integral_constant<int, 7>{});   // (what is left of the longest lists)
#undef V4_F_BIG
#undef V4_F_RING
#undef V4_F_SOFF
#undef V4_F_EDGE
#undef V4_F_TAG
#undef V4_F_SROW
#undef V4_F_SGR
#undef V4_F_CC
#undef V4_F_CP
#undef V4_F_GD
#undef V4_SCAN_STEP
#undef V4_FENCE
                        if (bP && __builtin_expect(UNI(TAGOF(fP)) != tagx, 0)) {
                            // not there yet: wait for the fetcher to deliver it (bounded by a time-out that flags the job; once it
                            // is flagged the remaining rows of the group run through without waiting)
                            DG_T0()
                            const unsigned t0 = V3_TICKS();
                            for (unsigned spin = 1; !dead; ++spin) {
                                // (polling the neighbour's global words directly here instead was measured: no faster)
                                fP = LLD(ringP[r]);
                                if (UNI(TAGOF(fP)) == tagx) break;
                                // time-out: the job is flagged and the loop left after this row -- which is finished with whatever
                                // is there, nobody will look at the result
                                if ((spin & 1023u) == 0 && (V3_TICKS() - t0 > V3_TIMEOUT_TICKS || UNI(GLD(abortf)))) { dead = true; break; }
                                __builtin_amdgcn_s_sleep(1);
                            }
                            DG_ADD(dg_wait_fast)
                        }
                        const int P_in_v = bP ? (int)(unsigned)fP : PWR_BIG;
                        const int P_end_v = min(P_in_v, incl);
                        const int pq = min(P_in_v, FBIG);
                        // (the word to publish is put together here, not inside the one-lane store: its two instructions are the wait
                        // states between the scan's result and the shift that reads it)
                        typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
                        v2u_ w2_; w2_.x = (unsigned)P_end_v; w2_.y = tagx;
                        if (!WG1 && CLS != 2) asm volatile("" : "+v"(w2_));        // (LEFT publishes the scan's result as it stands: pinning the pair would cost it a move)
                        int p = min(__builtin_amdgcn_update_dpp(pq, incl, DPP_WAVE_SHR1, 0xF, 0xF, false), pq);
#pragma unroll
                        for (int i = 0; i < C; ++i) {
                            if (BITS) accA[i] = acc_push(accA[i], __builtin_amdgcn_sicmp(tg[i], p, ICMP_SGE));
                            p = min(p, tg[i]);
                            // N = p: no band guard, so p <= tg[i] <= ig[i] already; behind a guard tg[i] may be FBIG
                            // (a RIGHT row without its clamp was measured and is NOT in the code: no proof for rows with blank runs)
                            Mprev[i] = (unsigned)(CLS == 0 ? p : min(p, ig[i]));
                        }
                        mlast_v = (unsigned)fP;                                     // M_last(x) = P_end(x) wherever the next row reads it
                        if (lane == 63) {
                            if (WG1) {
                                GST2(gq0 + r, P_end_v, tagx);
                                LST(rP[wr][(g0 + r) & (RB - 1)], ((unsigned long long)tagx << 32) | (unsigned)P_end_v);
                            } else {
                                // (sc1 as the agent-scope atomic stores have it: the word must be seen by the other work-groups; a store
                                // of 64 bits needs no wait states before a VALU overwrites its data registers)
                                // (the group's base is wave-uniform: scalar base + the row's byte offset, one move instead of 64-bit address arithmetic)
                                asm volatile("global_store_dwordx2 %0, %1, %2 sc1" :: "v"(8 * r), "v"(w2_), "s"(gq0) : "memory");
                            }
                        }
                    };
                    int r_end = r_e;
                    DG_T2()
                    // Code size matters (a straight-line copy per role and per entry row outgrew the instruction cache: every row
                    // 30 % slower, measured), and so does straight-line code (a one-row loop body costs 1.5x per row, measured).
                    // So: whole INTERIOR groups as 16 rows of straight-line code; everything else in blocks of 4 rows per role,
                    // aligned to 4 -- the band's leading strip, which sets the pace of the whole pipeline, is LEFT for only ~28
                    // rows at a time and would otherwise spend most of them in the one-row loop --, and that loop for the rest.
                    using WithBits = std::integral_constant<bool, true>;
                    using NoBits = std::integral_constant<bool, false>;
                    const bool warmup = (x >> 4) < g_own;                          // (the group lies in the warm-up: its record is not kept)
                    if (warmup && r_beg == 0 && r_e == 16 && cls != 3) {
                        // whole groups of the warm-up -- seven rows in ten of a segment --, one role: the same straight-line code without
                        // the two compare-and-shift pairs per cell that make the record
                        if (cls == 0) {
                            guard_head(0, std::integral_constant<int, PWR_INTERIOR_CLS>{});
#pragma unroll
                            for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, PWR_INTERIOR_CLS>{}, NoBits{});
                            DG_INC(dg_int, 16)
                            DG_ADD2(dg_cyc_int)
                        } else if (cls == 1) {
                            guard_head(0, std::integral_constant<int, 1>{});
#pragma unroll
                            for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, 1>{}, NoBits{});
                        } else {
                            guard_head(0, std::integral_constant<int, 2>{});
#pragma unroll
                            for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, 2>{}, NoBits{});
                        }
                    } else if (cls == 0 && r_beg == 0 && r_e == 16) {
                        guard_head(0, std::integral_constant<int, PWR_INTERIOR_CLS>{});
#pragma unroll
                        for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, PWR_INTERIOR_CLS>{}, WithBits{});
                        DG_INC(dg_int, 16)
                        DG_ADD2(dg_cyc_int)
                    } else if (cls == 1 && r_beg == 0 && r_e == 16) {
                        // (the band's last strip: its wave has just taken it over and the next strip's wave is waiting for it --
                        // this is the pipeline's critical path, so whole groups get straight-line code here too)
                        guard_head(0, std::integral_constant<int, 1>{});
#pragma unroll
                        for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, 1>{}, WithBits{});
                    } else if (cls == 3 && r_beg == 0 && r_e == 16) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, 3>{}, WithBits{});
                    } else if (cls == 2 && r_beg == 0 && r_e == 16) {
                        // (the band's first strip: with every follower close behind its neighbour, its rows set the pace)
                        guard_head(0, std::integral_constant<int, 2>{});
#pragma unroll
                        for (int r = 0; r < 16; ++r) group_row(r, std::integral_constant<int, 2>{}, WithBits{});
                    } else {
                        int r = r_beg;
                        for (; r < r_end && (r & 3) && !dead; ++r) group_row(r, std::integral_constant<int, 3>{}, WithBits{});
#define V4_BLOCKS(K) guard_head(r, std::integral_constant<int, K>{}); for (; r + 4 <= r_end && !dead; r += 4) { group_row(r, std::integral_constant<int, K>{}, WithBits{}); group_row(r + 1, std::integral_constant<int, K>{}, WithBits{}); \
                                                               group_row(r + 2, std::integral_constant<int, K>{}, WithBits{}); group_row(r + 3, std::integral_constant<int, K>{}, WithBits{}); }
                        if (cls == 0) { V4_BLOCKS(0) }
                        else if (cls == 1) { V4_BLOCKS(1) }
                        else if (cls == 2) { V4_BLOCKS(2) }
#undef V4_BLOCKS
                        for (; r < r_end && !dead; ++r) group_row(r, std::integral_constant<int, 3>{}, WithBits{});
                        r_end = r;
                    }
                    if (!(cls == 0 && r_beg == 0 && r_e == 16)) { DG_INC(dg_gen16, r_end - r_beg) DG_ADD2(dg_cyc_gen16) }
                    x = g0 + r_end;
#ifdef PWR_DIAG
                    if (lane == 0 && dg_me && dg_log < 1270) {
                        unsigned long long *lg = jb.diag + ((size_t)job * 32 + wave) * 4096 + 256 + 3 * dg_log;
                        lg[0] = (unsigned long long)x | ((unsigned long long)(cls | (warmup ? 16 : 0)) << 32) | ((unsigned long long)(r_end - r_beg) << 40); lg[1] = __builtin_amdgcn_s_memrealtime();
                        lg[2] = dg_wait_fast + dg_wait_gen + dg_wait_setup;
                    }
                    dg_log += 1;
#endif
                    af_done = __builtin_amdgcn_readlane(dcaf, (x - 1) & 63);       // anf of the last row done
                    if ((x & 15) == 0) {                                          // the 16-row group is complete
                        uint32_t *d_ = dirs + (size_t)gacc * RS + (size_t)wave * MS + (size_t)lc;
#pragma unroll
                        for (int i = 0; i < C; ++i) { if (gacc >= g_own) d_[i] = accA[i] | (accC[i] << 16); accA[i] = accC[i] = 0; }
                        gacc = -1; nacc = 0;
                        V4_CHK_STORE(x, af_done, min(af_done + B, W))
                    } else nacc = x & 15;
                    if (dead || x >= Lf) break;
                    if ((x >> 6) != blk) {
                        V4_ROTATE_BLOCK()
                        bOm = __builtin_amdgcn_ballot_w64((dcf & 1u) != 0); bPm = __builtin_amdgcn_ballot_w64((dcf & 2u) != 0);
                        bMm = __builtin_amdgcn_ballot_w64((dcf & 4u) != 0); bTm = __builtin_amdgcn_ballot_w64((dcf & 8u) != 0);
                        V4_EARLY_MASKS()
                        dcaf = (int)(dca & 0xffffffu); dcb = min(dcaf + B, W);
                        dcs = min(dca >> 24, 3u) * (unsigned)(MS * 4);
                        g_cp = -1;
                        const int *const srow0 = (const int *)(stab + __builtin_amdgcn_readlane((int)dcs, 0));
#pragma unroll
                        for (int i = 0; i < C; ++i) sgr[i] = srow0[i];
                    }
                    if (lane == 0) LST(wprog[lw], x);
                }
                a_prev = af_done; Bx_prev = min(B, W - af_done);
                if (dead) break;
                if (x < L) {
                    if ((x >> 6) != blk) V4_ROTATE_BLOCK()
                    a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
                    sx = __builtin_amdgcn_readlane(scur, x & 63);
                }
                if (lane == 0) LST(wprog[lw], x);
                continue;
            }
        }
        if (dead || x >= L) break;

        // ---- general path: one row, or one change of macro-strip
        x = UNI(x); ms = UNI(ms); msn = UNI(msn); a = UNI(a); a_prev = UNI(a_prev); Bx_prev = UNI(Bx_prev);
        sx = UNI(sx); gacc = UNI(gacc); nacc = UNI(nacc); blk = UNI(blk); gleft = UNI(gleft); gleftn = UNI(gleftn); ran_prev = UNI(ran_prev); cs = UNI(cs);
        const int Bx = min(B, W - a);
        const int ms_lo = (a - lo) / MS, ms_hi = (a + Bx - 1 - lo) / MS;
        if (ms < ms_lo) {
            ms += NW;
            if (ms == msn) {
#pragma unroll
                for (int i = 0; i < C; ++i) { ug[i] = nu[i]; gg[i] = ng[i]; ig[i] = ni[i]; }
                gleft = gleftn;
                cs ^= 1;
            } else {
                while (ms < ms_lo) ms += NW;
                V4_LOADS(ms, cs, ug, gg, ig, gleft)
            }
            DG_INC(dg_switch, 1)
            msn = ms + NW;
            V4_LOADS(msn, cs ^ 1, nu, ng, ni, gleftn)
            ran_prev = 0;
            continue;
        }
        if (ms > ms_hi) {
            // No work for this wave in row x: the band has not reached its macro-strip yet.  Skip to the first row of this
            // 64-row block whose band end lies beyond the strip's first column (or to the next block) in one step -- with
            // more macro-strips than the band is wide (NW * MS > B + MS) a wave spends whole laps here.
            const int y0s = lo + ms * MS;
            const int anf_l = (int)(dca & 0xffffffu);                             // lane = row of this 64-row block
            const unsigned long long wm = __builtin_amdgcn_ballot_w64(min(anf_l + B, W) > y0s) >> (x & 63);
            const int xn = min(wm ? x + __builtin_ctzll(wm) : ((x >> 6) + 1) << 6, L);     // (> x: row x itself has no work)
            // (take the strip over at the group boundary before xn, see V4_EARLY_MASKS; the fast path starts it)
            int xs = xn;
            if (wm && xn < Lf) {
                // A TEAR is a row whose band starts at or beyond the end of the band of the row above (the row's next base lies
                // more than a bandwidth further right: a run of blanks between two of its segments).  No strip is taken over
                // across one: the waves of the strips the band jumps over never run the rows in between, so nobody would hand
                // anything over there -- the rows run ahead start at the last tear up to xn at the earliest (every wave applies
                // the same rule, so a wave's rows ahead are always covered by its left neighbour's).  And a strip the band
                // jumps over altogether in row xn is not started at all: the general path changes strips first.
                const int anf_up = __builtin_amdgcn_update_dpp(0x3fffffff, anf_l, DPP_WAVE_SHR1, 0xF, 0xF, false);
                const unsigned long long tears = __builtin_amdgcn_ballot_w64(anf_l >= min(anf_up + B, W)) >> (x & 63);   // bit i: row x + i
                const unsigned long long tm = tears & (~0ull >> (63 - (xn - x))) & ~1ull;                              // rows (x, xn]
                xs = max(x, xn & ~15);
                if (tm) xs = max(xs, x + 63 - __builtin_clzll(tm));
                if (xs < 1) xs = xn;
                const int an = __builtin_amdgcn_readlane(anf_l, xn & 63);
                if (ms < (an - lo) / MS) { xs = xn; first_pending = 0; }
                else { early_lo = xs; early_hi = xn; first_pending = xs > 0 ? 1 : 0; }
            }
            DG_INC(dg_nowork, xs - x)
            if (xs > x) {
                const int al = __builtin_amdgcn_readlane((int)dca, (xs - 1) & 63) & 0xffffff;  // row xs - 1 is in this block
                a_prev = al; Bx_prev = min(B, W - al);
            }
            x = xs;
            ran_prev = 0;
            if (lane == 0) LST(wprog[lw], x);
            if (x < L) {
                if ((x >> 6) != blk) V4_ROTATE_BLOCK()
                a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
                sx = __builtin_amdgcn_readlane(scur, x & 63);
            }
            continue;
        }
        if (!ran_prev && x > 0 && x < Lf) { first_pending = 1; continue; }        // first row on this macro-strip: the fast path takes it
        const int y0 = lo + ms * MS;
        const int yq = y0 - 1;
        const bool needP = ms > ms_lo;
        const bool needM = x > 0 && yq >= a_prev && yq < a_prev + Bx_prev;
        const bool needT = x > 0 && ((yq >= a_prev + Bx_prev) || !ran_prev);
        unsigned ePx = 0, ePy = 0, eMy = 0, eTx = 0;
        if (WG1 && x - RB + 2 > 0) {
            const unsigned t0 = V3_TICKS();
            for (unsigned spin = 1; UNI(LLD(wprog[wr])) < x - RB + 2; ++spin) {
                if ((spin & 1023u) == 0 && (V3_TICKS() - t0 > V3_TIMEOUT_TICKS || UNI(GLD(abortf)))) { dead = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (dead) break;
        }
        {
            const unsigned tagx = tagbase | (unsigned)(x + 1), tagp = tagbase | (unsigned)x;
#ifdef PWR_DIAG
            const unsigned long long ev_t0 = __builtin_amdgcn_s_memrealtime();
#endif
            DG_T0()
            const unsigned t0 = V3_TICKS();
            for (unsigned spin = 1;; ++spin) {
                // (the neighbour's last column lies in the band of row x where needP, of row x - 1 where needM: its score there is
                // the P_end word itself)
                const unsigned long long eP = LLD(rP[lw][x & (RB - 1)]);
                const unsigned long long eM = LLD(rP[lw][(x - 1) & (RB - 1)]), eT = needT ? GLD(PTOT_PTR(a_prev, Bx_prev, x - 1)) : 0ull;
                ePx = UNI((unsigned)eP); ePy = ePx; eMy = UNI((unsigned)eM); eTx = UNI((unsigned)eT);
                const bool ready = (!needP || UNI(TAGOF(eP)) == tagx) &&
                                   (!needM || UNI(TAGOF(eM)) == tagp) && (!needT || UNI(TAGOF(eT)) == tagp);
                if (ready) break;
                if ((spin & 1023u) == 0 && (V3_TICKS() - t0 > V3_TIMEOUT_TICKS || UNI(GLD(abortf)))) { dead = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
#ifdef PWR_DIAG
            if (lane == 0 && dg_me && dg_general < 36) {
                unsigned long long *ev = jb.diag + ((size_t)job * 32 + wave) * 4096 + 16 + 3 * dg_general;
                ev[0] = (unsigned long long)x; ev[1] = ev_t0; ev[2] = __builtin_amdgcn_s_memrealtime();
            }
#endif
            DG_ADD(dg_wait_gen)
            DG_INC(dg_general, 1)
            if (dead) break;
        }
        int Mleft = (int)PWR_INF;
        if (x == 0) Mleft = (src_c < 0 || yq == src_c) ? -gleft : (int)PWR_INF - gleft;
        else if (yq < a_prev) Mleft = (int)PWR_INF - gleft;                      // PW:276
        else if (needM) Mleft = (int)eMy;
        else Mleft = (int)eTx;                                                   // PW:285-295
        const int P_in = needP ? (int)ePx : PWR_BIG;
        if (x > 0 && !ran_prev) {
#pragma unroll
            for (int i = 0; i < C; ++i) Mprev[i] = eTx;
        }
        if ((x >> 4) != gacc) { V4_FLUSH() gacc = x >> 4; }
        V4_ALIGN_ACC(x & 15)
        const int pm1_0 = __builtin_amdgcn_update_dpp(Mleft, (int)Mprev[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);
        const int sxc = min(max(sx, 0), 3);                                      // PW:1503 Score(y, Seq_Bases[x])
        const int rel0 = y0 + lc - a;
        int tg[C];
        int run = PWR_BIG;
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int pm1 = i ? (int)Mprev[i > 0 ? i - 1 : 0] : pm1_0;
            const int d = pm1 + ldsS1[lw][cs][sxc][lc + i];
            const int u = (int)Mprev[i] + ug[i];
            accC[i] = (accC[i] << 1) | ((d <= u) ? 1u : 0u);
            const int t3 = min(min(d, u), ig[i]);
            tg[i] = ((unsigned)(rel0 + i) < (unsigned)Bx) ? t3 : PWR_BIG;
            run = min(run, tg[i]);
        }
        const int incl = wave_incl_min(run);
        const int excl = __builtin_amdgcn_update_dpp(PWR_BIG, incl, DPP_WAVE_SHR1, 0xF, 0xF, false);
        const int P_end = min(P_in, __builtin_amdgcn_readlane(incl, 63));
        int p = min(P_in, excl);
        if (x != Lf) {
#pragma unroll
            for (int i = 0; i < C; ++i) {
                accA[i] = (accA[i] << 1) | ((tg[i] >= p) ? 1u : 0u);
                p = min(p, tg[i]);
                Mprev[i] = (unsigned)((rel0 + i < 0) ? ig[i] : p);
            }
        } else {
            // (the DP's last row: only the job's last segment gets here with x == Lf)
            // (the scores leave the kernel here: Mn is the true M = G + N, as lastM and the test of PW:1386 want it)
            unsigned Mn[C];
            unsigned fa = 0;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                fa |= (tg[i] >= p) ? (1u << i) : 0u;
                p = min(p, tg[i]);
                Mn[i] = (rel0 + i < 0) ? PWR_INF : (unsigned)(gg[i] + p);
                Mprev[i] = (unsigned)((rel0 + i < 0) ? ig[i] : p);
            }
            const unsigned mrow = needP ? (unsigned)gleft + ePy : PWR_INF;
            const unsigned left0 = (unsigned)__builtin_amdgcn_update_dpp((int)mrow, (int)Mn[C - 1], DPP_WAVE_SHR1, 0xF, 0xF, false);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const unsigned lf = i ? Mn[i > 0 ? i - 1 : 0] : left0;
                const bool inb = (unsigned)(rel0 + i) < (unsigned)Bx;
                accA[i] = (accA[i] << 1) | ((((fa >> i) & 1u) || (inb && Mn[i] == lf)) ? 1u : 0u);
                lastM[wave * MS + lc + i] = inb ? Mn[i] : 0xffffffffu;
            }
        }
        nacc = (x & 15) + 1;
        if (lane == 63) {
            GST(gmy + (size_t)x, P_end, x);
            if (WG1) LST(rP[wr][x & (RB - 1)], ((unsigned long long)(tagbase | (unsigned)(x + 1)) << 32) | (unsigned)P_end);
        }
        ran_prev = 1;
        V4_CHK_STORE(x + 1, a, a + Bx)
        V4_NEXT_ROW()
    }
    V4_FLUSH()
#ifdef PWR_DIAG
    if (lane == 0 && dg_me) {
        unsigned long long *dgp = jb.diag + ((size_t)job * 32 + wave) * 4096;
        dgp[0] = __builtin_amdgcn_s_memtime() - t_clk0; dgp[1] = dg_wait_fast; dgp[2] = dg_wait_gen; dgp[3] = dg_wait_setup;
        dgp[4] = ((unsigned long long)dg_int << 32) | dg_gen16; dgp[5] = ((unsigned long long)dg_general << 32) | dg_nowork;
        dgp[6] = ((unsigned long long)dg_runs << 32) | dg_switch; dgp[7] = (unsigned long long)L;
        dgp[12] = dg_log; dgp[8] = dg_cyc_gen16; dgp[9] = dg_ts1; dgp[10] = dg_ts2; dgp[11] = dg_cyc_int;
    }
#endif
#ifdef PWR_DIAG
    if (lane == 0 && sd->s * NW + wave < 680) { tl[3] = __builtin_amdgcn_s_memrealtime(); tl[4] = (unsigned long long)L | ((unsigned long long)(dg_wait_fast + dg_wait_gen + dg_wait_setup) << 20); }
#endif
    if (lane == 0) { LST(wprog[lw], 0x7fffffff); LST(wdone, 1); }                     // releases the left neighbour / the fetcher
    if (dead) {
        // A wave gave up waiting (its neighbour's work-group is not running: the GPU is shared, or more contexts are in
        // flight than it can hold at once).  The job is flagged -- its siblings leave, trace and commit skip it -- and the
        // commit kernel switches the next batches to k_fill_v2, which needs no other work-group (Hdr::fallback).
        if (lane == 0) __hip_atomic_store(abortf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (wave == 0 && lane == 0) {
        if (sd->s == 0) {
            m->clk = (unsigned)(__builtin_amdgcn_s_memtime() - t_clk0);
            m->rclk = (unsigned)(__builtin_amdgcn_s_memrealtime() - t_real0);
            m->rounds = 0;
        }
        atomicAdd(&st.hdr->cells_computed, sd->cells);
    }
#undef V4_CHK_STORE
#undef V4_EARLY_MASKS
#undef PTOT_PTR
#undef GLD
#undef GST
#undef GST2
#undef TAGOF
#undef LLD
#undef LST
#undef V4_LOADS
#undef V4_ALIGN_ACC
#undef V4_FLUSH
#undef V4_ROTATE_BLOCK
#undef V4_NEXT_ROW
}

// ---------------------------------------------------------------------------------------------
// The check behind the segmented fill: segment s (s > 0) started from a start of its own some hundred rows before its own part;
// its record is the true one iff, in the row before its own part, its scores are PARALLEL to the ones segment s - 1 ends on:
// the same cells unreachable (>= PWR_INF) and one and the same difference in every other cell of the band -- a min-plus
// recurrence maps parallel rows to parallel rows, and every bit of the record compares two candidates of one row.  (By
// induction the scores segment s - 1 ends on are themselves parallel to the true ones.)  One work-group per (job, s); the
// entries are consumed (set to "not written"), so a store that went missing can never pass for a match.
// ---------------------------------------------------------------------------------------------
// (does this job's fill have boundaries to check in this batch?  -- one rule for the check and for whoever waits for it)
__device__ __forceinline__ bool seg_check_applies(const DState &st, const JobBufs &jb, int job, const JobMeta *m)
{
    return m->active && m->L > 0 && m->ok && !m->wide && !m->abort && !(st.hdr->fallback > 0 && jb.v2_follows) && !NOT_MINE(jb, job) && m->nseg > 1;
}

// one work-group of 256 threads per (job, boundary s); `chkdone[job]` counts the boundaries done (for the traceback kernel, which
// carries these work-groups in its own launch and must know when the verdict is in before it reports an inconsistent record)
__device__ __forceinline__ void seg_check_body(const DState &st, const JobBufs &jb, const int job, const int s, const int tid)
{
    __shared__ int s_min[4], s_max[4], s_bad;
    JobMeta *m = &jb.meta[job];
    if (!seg_check_applies(st, jb, job, m)) return;
    if (s >= m->nseg) return;
    const SegDesc *sd = jb.seg + (size_t)job * SEG_MAX + s;
    const int xr = sd->xown - 1;                                                   // the row both segments have
    const int lo = m->lo, W = m->W, B = st.B, H = st.H, RS = jb.NC;
    const int a = max(0, jb.way[(size_t)job * jb.Lmax + xr] - H), Bx = min(B, W - a);
    unsigned *cw = jb.chk + (((size_t)job * (SEG_MAX + 1) + s) * 2 + 0) * (size_t)jb.NC;
    unsigned *ct = jb.chk + (((size_t)job * (SEG_MAX + 1) + s) * 2 + 1) * (size_t)jb.NC;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int dmin = INT_MAX, dmax = INT_MIN, bad = 0;
    for (int j = tid; j < Bx; j += 256) {
        const int idx = (a + j - lo) % RS;
        const unsigned vw = cw[idx], vt = ct[idx];
        if (vw == 0xffffffffu || vt == 0xffffffffu) bad = 1;                       // a band cell nobody stored
        else if ((vw >= PWR_INF) != (vt >= PWR_INF)) bad = 1;
        else if (vw < PWR_INF) { const int d = (int)(vw - vt); dmin = min(dmin, d); dmax = max(dmax, d); }
    }
    for (int o = 32; o > 0; o >>= 1) { dmin = min(dmin, __shfl_xor(dmin, o)); dmax = max(dmax, __shfl_xor(dmax, o)); }
    if ((tid & 63) == 0) { s_min[tid >> 6] = dmin; s_max[tid >> 6] = dmax; }
    if (bad) s_bad = 1;
    __syncthreads();
    // the entries are consumed -- the WHOLE strip, not only the band cells read: a later fill that skips a store must meet
    // "not written", never a finite value left over from an earlier launch
    for (int j = tid; j < RS; j += 256) { cw[j] = 0xffffffffu; ct[j] = 0xffffffffu; }
    if (tid == 0) {
        const int lo_ = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3])), hi_ = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (s_bad || (lo_ != INT_MAX && lo_ != hi_)) __hip_atomic_store(&m->segfail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s == 1) { atomicAdd(&st.hdr->seg_jobs, 1ull); atomicAdd(&st.hdr->segs, (unsigned long long)m->nseg); }
        __hip_atomic_fetch_add(&jb.chkdone[job], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_seg_check(DState st, JobBufs jb)
{
    seg_check_body(st, jb, (int)blockIdx.x, (int)blockIdx.y + 1, (int)threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// fill, 64-bit fallback (the reference's own arithmetic: unsigned long Matrix, INF = ULONG_MAX/2, PW:30, PW:271).  Taken
// per job when the gather cannot prove that the scores of the row fit the 32-bit wave pipeline (very deep stacks: the
// bound is cost of the present placement + (2B + 4096) x the largest tally >= 2^30, or 2^29 bases in the interval).  One
// work-group per job, two band cells per thread, tallies read straight from the state, the in-row dependency as the same
// min-plus scan (block-wide, 64-bit); output in the layout the traceback kernels read: two bits per cell, and the last
// row's scores RELATIVE to their minimum (the entry scan of PW:1352-1360 only compares them), saturated at 2^32 - 2.
// Slow (two barriers per DP row) and never on the benchmark path.
// ---------------------------------------------------------------------------------------------
#define F64_NT 1024
#define F64_INF (1ll << 62)
__global__ __launch_bounds__(F64_NT) void k_fill64(DState st, JobBufs jb)
{
    __shared__ long long prevM[2][2 * F64_NT + 2];          // DP rows x-1 / x, band-relative
    __shared__ long long wtot[F64_NT / 64];
    __shared__ long long s_lastcell[2], s_min;
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    JobMeta *m = &jb.meta[job];
    const int L = m->L;
    if (!m->active || L <= 0 || !m->ok || !m->wide || NOT_MINE(jb, job)) return;
    const int lo = m->lo, hi = m->hi, W = m->W, B = st.B, H = st.H, RS = jb.NC;
    const int n = hi - lo + 1;
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const uint8_t *seq = st.seq + st.rowoff[m->k];
    const uint8_t *mark = jb.mark + (size_t)job * jb.colcap;
    const int *order = cur_order(st);
    uint32_t *dirs = jb.dirs + (size_t)job * jb.dirstride;
    unsigned *lastM = jb.lastM + (size_t)job * jb.NC;
    long long *G = jb.g64 + (size_t)job * jb.colcap;          // G[i] = sum_{j <= i} S(lo + j, 4), row removed
    const int way0 = way[0], wayL = way[L - 1];
    // tallies of column y with the row's own symbol taken out (Columns_Downdater, PW:1172-1201)
    auto tally_of = [&](int y, uint32_t *w) {
        const Tally t = st.tally[order[y]];
#pragma unroll
        for (int b = 0; b < 6; ++b) w[b] = t.w[b];
        if (y >= way0 && y <= wayL) {
            const int mk = mark[y - lo];
            const int own = mk == 7 ? 5 : (mk ? mk - 1 : 4);
#pragma unroll
            for (int b = 0; b < 6; ++b) w[b] -= (own != 5 && b != own) ? 1u : 0u;
        }
    };
    // ---- prefix sums of S(.,4) over the interval, traceback words cleared, last-row slots marked unused
    {
        long long carry = 0;
        for (int base = 0; base < n; base += F64_NT) {
            const int i = base + tid;
            long long v = 0;
            if (i < n) { uint32_t w[6]; tally_of(lo + i, w); v = (long long)w[4]; }
            long long incl = v;
            for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
            if (lane == 63) wtot[wv] = incl;
            __syncthreads();
            long long pre = 0, tot = 0;
            for (int w = 0; w < F64_NT / 64; ++w) { const long long s = wtot[w]; pre += (w < wv) ? s : 0; tot += s; }
            __syncthreads();
            if (i < n) G[i] = carry + pre + incl;
            carry += tot;
        }
        const size_t nwords = (size_t)((L + 15) / 16) * RS;
        for (size_t i = tid; i < nwords; i += F64_NT) dirs[i] = 0;
        for (int i = tid; i < RS; i += F64_NT) lastM[i] = 0xffffffffu;
        __syncthreads();
    }
    auto Gat = [&](int y) -> long long { return y < lo ? 0 : G[y - lo]; };      // (y >= lo - 1 always)
    int a_prev = 0, B_prev = 0;
    for (int x = 0; x < L; ++x) {
        const int a = max(0, way[x] - H), Bx = min(B, W - a);                    // PW:1496-1497
        const int sx = seq[x];
        const long long *pv = prevM[(x & 1) ^ 1];
        long long *cur = prevM[x & 1];
        const long long plast = s_lastcell[(x & 1) ^ 1];                         // M[x-1][B-1], for the extension of PW:285-295
        // Out(x-1, y), PW:249-303
        auto out_prev = [&](int y) -> long long {
            if (x == 0) return 0;
            if (y < 0 || y < a_prev) return F64_INF;
            if (y >= a_prev + B_prev) return plast >= F64_INF ? F64_INF : plast + Gat(y) - Gat(a_prev + B_prev - 1);
            return pv[y - a_prev];
        };
        long long tg[2], gy[2];
        bool cbit[2], inb[2];
        long long run = F64_INF;                                                 // min over this thread's cells of t - G
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = 2 * tid + i, y = a + j;
            inb[i] = j < Bx;
            tg[i] = F64_INF; gy[i] = 0; cbit[i] = false;
            if (inb[i]) {
                uint32_t w[6];
                tally_of(y, w);
                long long d = out_prev(y - 1);
                d = d >= F64_INF ? F64_INF : d + (long long)w[sx < 4 ? sx : 3];   // PW:1503
                long long u = F64_INF;
                if (y > 0 && y < W - 1) {                                         // PW:1505
                    uint32_t wl[6];
                    tally_of(y - 1, wl);
                    const long long o = out_prev(y);
                    u = o >= F64_INF ? F64_INF : o + (long long)max(w[5], wl[5]); // PW:1507
                }
                cbit[i] = d <= u;
                tg[i] = min(d, u);
                gy[i] = G[y - lo];
                run = min(run, tg[i] >= F64_INF ? F64_INF : tg[i] - gy[i]);
            }
        }
        // exclusive block prefix-min of (t - G) in band order
        long long incl = run;
        for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl = min(incl, t); }
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        long long pre = F64_INF;
        for (int w = 0; w < wv; ++w) pre = min(pre, wtot[w]);
        long long excl = __shfl_up(incl, 1);
        if (lane == 0) excl = F64_INF;
        long long p = min(pre, excl);
        unsigned abits = 0;
        long long Mv[2] = {F64_INF, F64_INF};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (inb[i]) {
                const long long q = tg[i] >= F64_INF ? F64_INF : tg[i] - gy[i];
                if (q >= p) abits |= 1u << i;                                     // PW:1375: M equals the left candidate
                p = min(p, q);
                Mv[i] = p >= F64_INF ? F64_INF : p + gy[i];
            }
        }
        if (x == L - 1) {
            // PW:1386: on the last row a cell that merely EQUALS its left neighbour is a (blank) left move too
            long long leftv = __shfl_up(Mv[1], 1);
            if (lane == 0) leftv = F64_INF;
            // (the neighbour wave's last cell: through LDS)
            cur[2 * tid] = Mv[0]; cur[2 * tid + 1] = Mv[1];
            __syncthreads();
            if (tid > 0) leftv = cur[2 * tid - 1];
            if (inb[0] && Mv[0] == leftv) abits |= 1u;
            if (inb[1] && Mv[1] == Mv[0]) abits |= 2u;
        } else {
            cur[2 * tid] = Mv[0]; cur[2 * tid + 1] = Mv[1];
        }
        if (2 * tid == ((Bx - 1) & ~1)) s_lastcell[x & 1] = Mv[(Bx - 1) & 1];
        // traceback bits: word (x / 16, (y - lo) mod RS), A at bit 15 - x % 16, C at bit 31 - x % 16
        const int sh = 15 - (x & 15);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (inb[i]) {
                const unsigned v = (((abits >> i) & 1u) << sh) | ((cbit[i] ? 1u : 0u) << (16 + sh));
                if (v) atomicOr(&dirs[(size_t)(x >> 4) * RS + (size_t)((a + 2 * tid + i - lo) % RS)], v);
            }
        }
        a_prev = a; B_prev = Bx;
        __syncthreads();
    }
    // ---- last row, relative to its minimum
    {
        const long long *lr = prevM[(L - 1) & 1];
        const int a = a_prev, Bx = B_prev;
        long long mn = F64_INF;
        for (int j = tid; j < Bx; j += F64_NT) mn = min(mn, lr[j]);
        for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o));
        if (lane == 0) wtot[wv] = mn;
        __syncthreads();
        if (tid == 0) { long long r = F64_INF; for (int w = 0; w < F64_NT / 64; ++w) r = min(r, wtot[w]); s_min = r; }
        __syncthreads();
        const long long r = s_min;
        for (int j = tid; j < Bx; j += F64_NT) {
            const long long v = lr[j] >= F64_INF ? (long long)0xfffffffeu : min(lr[j] - r, (long long)0xfffffffeu);
            lastM[(a + j - lo) % RS] = (unsigned)v;
        }
    }
    if (tid == 0) atomicAdd(&st.hdr->cells_computed, m->cells);
}

// ---------------------------------------------------------------------------------------------
// trace for the wave-pipeline layout (dirs indexed by (y - lo) mod RS, the same word for a column
// in every row of a 16-row group).  Also picks the entry column (PW:1352-1360) from lastM.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_trace_wp(DState st, JobBufs jb)
{
    const int job = blockIdx.x, lane = threadIdx.x;
    JobMeta *m = &jb.meta[job];
    const int L = UNI(m->L);
    if (!m->active || L <= 0 || !m->ok || m->abort || m->segfail || (m->wide && !jb.f64_follows) || NOT_MINE(jb, job)) return;   // (not filled: stalled, failed its check, or its batch came without k_fill64)
    const int W = UNI(m->W), B = st.B, H = st.H, RS = jb.NC, lo = UNI(m->lo);
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const uint32_t *dirs = jb.dirs + (size_t)job * jb.dirstride;
    const unsigned *lastM = jb.lastM + (size_t)job * jb.NC;
    int *newcol = jb.newcol + (size_t)job * jb.Lmax;

    int x = L - 1, err = 0, nnew = 0;
    int y;
    {   // entry: minimum of the last row over y in [ylow, W-1], ties -> largest y; columns past the band
        // carry the value of the last band cell (PW:287)
        const int wx = way[x];
        const int a = max(0, wx - H), Bx = min(B, W - a);
        int ylow = max(-1, wx - H) + 1;
        if (ylow > W - 1) ylow = W - 1;
        unsigned long long key = ~0ull;
        for (int yy = max(ylow, a) + lane; yy < a + Bx; yy += 64) {
            const unsigned v = lastM[(yy - lo) % RS];
            const unsigned long long k2 = ((unsigned long long)v << 32) | (unsigned)(~(unsigned)yy);
            key = k2 < key ? k2 : key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o);
            key = other < key ? other : key;
        }
        const unsigned vmin = (unsigned)(key >> 32);
        int entry = (key == ~0ull) ? -1 : (int)(~(unsigned)key);
        if (a + B <= W - 1) {
            const unsigned lastval = lastM[(a + B - 1 - lo) % RS];
            if (entry < 0 || lastval <= vmin) entry = W - 1;
        }
        entry = UNI(entry);
        y = entry;
        if (lane == 0) m->entry = entry;
        if (entry < 0) err = 4;
    }
    int gcur = -1, yb = 0;
    uint32_t win[4] = {0, 0, 0, 0};
    int gpre = -1, ybpre = 0;
    uint32_t pre[4] = {0, 0, 0, 0};
    int blk = x >> 6;
    int wcur = way[min(blk * 64 + lane, L - 1)];
    int wnxt = way[max(blk * 64 - 64 + lane, 0)];
    int ncreg = 0;
    while (x >= 0 && !err) {
        x = UNI(x); y = UNI(y); blk = UNI(blk); gcur = UNI(gcur); yb = UNI(yb); gpre = UNI(gpre); ybpre = UNI(ybpre); nnew = UNI(nnew);
        // ---- fast path: rows of the current 16-row group / 64-row block whose answer lies in the
        //      64-cell sub-window holding the current column -- straight-line, no memory access
        while ((x >> 4) == gcur && (x >> 6) == blk) {
            const int af = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
            const int ycf = min(y, af + min(B, W - af) - 1);
            if (y < af || ycf < yb || ycf > yb + 255) break;
            const int q0 = (ycf - yb) >> 6, shf = 15 - (x & 15);
            const uint32_t wq = q0 == 0 ? win[0] : q0 == 1 ? win[1] : q0 == 2 ? win[2] : win[3];
            const int cy = yb + 64 * q0 + lane;
            const unsigned long long mk = __ballot(cy <= ycf && cy >= af && !((wq >> shf) & 1u));
            if (!mk) break;
            const int t = 63 - __builtin_clzll(mk);
            const int yy = yb + 64 * q0 + t;
            const int cb = (int)((__ballot((wq >> (16 + shf)) & 1u) >> t) & 1ull);
            ncreg = (lane == (x & 63)) ? ((yy << 1) | (cb ^ 1)) : ncreg;
            y = yy - cb;                                        // diag: column to the left, up: stay
            nnew += cb ^ 1;
            --x;
            if (x < 0 || y < 0) break;
        }
        if (x < 0) break;
        if (y < 0) { err = 3; break; }
        if ((x >> 6) != blk) {
            if (blk * 64 + lane < L) newcol[blk * 64 + lane] = ncreg;
            blk = x >> 6;
            wcur = wnxt;
            wnxt = way[max(blk * 64 - 64 + lane, 0)];
        }
        const int a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
        const int Bx = min(B, W - a);
        if (y < a) { err = 1; break; }
        int yc = min(y, a + Bx - 1);                         // past the band: implicit left moves
        const int g = x >> 4, sh = 15 - (x & 15);
        int found = -1, cbit = 0;
        for (;;) {
            if (g != gcur || yc < yb || yc > yb + 255) {
                const int want = max(lo, yc - 191);
                if (gpre == g && ybpre == want) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) win[q] = pre[q];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) win[q] = dirs[(size_t)g * RS + (want + 64 * q + lane - lo) % RS];
                }
                gcur = g; yb = want;
                if (g > 0) {
                    gpre = g - 1; ybpre = want;
#pragma unroll
                    for (int q = 0; q < 4; ++q) pre[q] = dirs[(size_t)(g - 1) * RS + (want + 64 * q + lane - lo) % RS];
                }
            }
            {   // common case: the answer lies in the 64-cell sub-window that holds yc
                const int q0 = (yc - yb) >> 6;
                const uint32_t wq = q0 == 0 ? win[0] : q0 == 1 ? win[1] : q0 == 2 ? win[2] : win[3];
                const int cy = yb + 64 * q0 + lane;
                const unsigned long long mk = __ballot(cy <= yc && cy >= a && !((wq >> sh) & 1u));
                if (mk) {
                    const int t = 63 - __builtin_clzll(mk);
                    found = yb + 64 * q0 + t;
                    const unsigned long long ck = __ballot((wq >> (16 + sh)) & 1u);
                    cbit = (int)((ck >> t) & 1ull);
                } else {
#pragma unroll
                    for (int q = 2; q >= 0; --q) {
                        if (found < 0 && q < q0) {
                            const int cy2 = yb + 64 * q + lane;
                            const unsigned long long mk2 = __ballot(cy2 >= a && !((win[q] >> sh) & 1u));
                            if (mk2) {
                                const int t = 63 - __builtin_clzll(mk2);
                                found = yb + 64 * q + t;
                                const unsigned long long ck = __ballot((win[q] >> (16 + sh)) & 1u);
                                cbit = (int)((ck >> t) & 1ull);
                            }
                        }
                    }
                }
            }
            if (found >= 0) break;
            if (yb <= a) { err = 2; break; }
            yc = yb - 1;
        }
        if (err) break;
        const int yy = found;
        if (cbit) { ncreg = (lane == (x & 63)) ? (yy << 1) : ncreg; y = yy - 1; }              // PW:1394 (c)
        else { ncreg = (lane == (x & 63)) ? ((yy << 1) | 1) : ncreg; y = yy; ++nnew; }         // PW:1404 (d)
        --x;
        if (x >= 0 && y < 0) { err = 3; break; }
    }
    if (!err && blk * 64 + lane < L) newcol[blk * 64 + lane] = ncreg;
    if (lane == 0) {
        m->nnew = nnew;
        m->changed = 1;                                       // (not worked out here: the commit takes the long way)
        if (err) { m->ok = 0; atomicCAS(&st.hdr->status, 0, PWR_ERR_INTERNAL); }
    }
}

// ---------------------------------------------------------------------------------------------
// trace, speculative-parallel form.  The traceback is a chain of L dependent steps, but its state
// between two DP rows is only the column the trace arrives at.  TRK waves each take a chunk of rows:
//   phase 0 (all waves at once): the top chunk starts from the true entry column; every other wave
//     GUESSES its arrival column (where the row above used to sit) and traces its chunk from there,
//     recording per row the arrival column and the placement;
//   phase 1 (top-down hand-over): when the chunk above is final its true exit column is known; if
//     the guess was right the chunk is final as it stands, otherwise the wave retraces from the true
//     column until it arrives at a row in the same column as the guess did -- from there on the
//     recorded steps are exactly the steps the true trace would make.  Optimal paths from nearby
//     columns merge within a few rows, so the hand-over chain is short.
// Results are those of k_trace_wp bit for bit (same per-row step; a step is a function of (row, column)).
// ---------------------------------------------------------------------------------------------
#define TRK 64                                          // chunks per job ...
#define TRW 4                                           // ... four to a work-group, so that the chunks of a job spread over four CUs
#define TR_SPIN_LIMIT (1 << 20)
// hand-over word of a chunk: [63:42] launch tag, [41:40] 1 = final / 2 = error, [39:24] its 'up' moves, [23:0] exit column + 1
#define TR_WORD(TAG, FLAG, CNT, Y) (((unsigned long long)(TAG) << 42) | ((unsigned long long)(FLAG) << 40) | ((unsigned long long)((CNT) & 0xffff) << 24) | (unsigned long long)(((Y) + 1) & 0xffffff))
__global__ __launch_bounds__(TRW * 64) void k_trace_par(DState st, JobBufs jb)
{
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = UNI((int)blockIdx.y * TRW + (tid >> 6));
    unsigned long long *const hand = jb.gtr + (size_t)job * jb.trk;
    const unsigned ttag = jb.trace_tag;
    JobMeta *m = &jb.meta[job];
    const int L = UNI(m->L);
    if (!m->active || L <= 0 || !m->ok || m->abort || m->segfail || (m->wide && !jb.f64_follows) || NOT_MINE(jb, job)) return;   // (not filled: stalled, failed its check, or its batch came without k_fill64)
    const int W = UNI(m->W), B = st.B, H = st.H, RS = jb.NC, lo = UNI(m->lo);
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const uint32_t *dirs = jb.dirs + (size_t)job * jb.dirstride;
    const unsigned *lastM = jb.lastM + (size_t)job * jb.NC;
    int *newcol = jb.newcol + (size_t)job * jb.Lmax;
    int *yin = jb.aux + (size_t)job * jb.Lmax;             // arrival column per row (aux is rewritten by the commit later)

    const int Lc = ((((L + TRK - 1) / TRK) + 63) >> 6) << 6;   // rows per chunk, a multiple of 64
    const int nch = (L + Lc - 1) / Lc;                      // chunks in use; chunk nch-1 holds the last DP row
    if (wv >= nch) return;
    const int x_lo = wv * Lc, x_top = min(L, x_lo + Lc) - 1;
    const bool top = (wv == nch - 1);

#ifdef PWR_DIAG
    const unsigned long long tr_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long tr_t1 = 0, tr_t2 = 0;
#endif
    int yguess = 0, yout_guess = 0, xrec_lo = x_top + 1;    // rows [xrec_lo, x_top] were recorded in phase 0
    int cnt = 0;                                            // 'up' moves (new columns) of the chunk as it stands
    int err = 0;
    for (int phase = 0; phase < 2; ++phase) {
        int x = x_top, y;
        bool check_merge = false;
        if (phase == 0) {
            if (top) {
                // entry: minimum of the last row over y in [ylow, W-1], ties -> largest y; columns past the
                // band carry the value of the last band cell (PW:287)
                const int wx = way[x];
                const int a = max(0, wx - H), Bx = min(B, W - a);
                int ylow = max(-1, wx - H) + 1;
                if (ylow > W - 1) ylow = W - 1;
                unsigned long long key = ~0ull;
                for (int yy = max(ylow, a) + lane; yy < a + Bx; yy += 64) {
                    const unsigned v = lastM[(yy - lo) % RS];
                    const unsigned long long k2 = ((unsigned long long)v << 32) | (unsigned)(~(unsigned)yy);
                    key = k2 < key ? k2 : key;
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long other = __shfl_xor(key, o);
                    key = other < key ? other : key;
                }
                const unsigned vmin = (unsigned)(key >> 32);
                int entry = (key == ~0ull) ? -1 : (int)(~(unsigned)key);
                if (a + B <= W - 1) {
                    const unsigned lastval = lastM[(a + B - 1 - lo) % RS];
                    if (entry < 0 || lastval <= vmin) entry = W - 1;
                }
                entry = UNI(entry);
                y = entry;
                if (lane == 0) m->entry = entry;
                if (entry < 0) { err = 4; break; }
            } else {
                y = UNI(way[x + 1]) - 1;                    // guess: just left of where the row above sits now
                yguess = y;
            }
        } else {
            if (top) break;                                 // already final
            unsigned long long hw = 0;
            int f = 0;
#ifdef PWR_DIAG
            tr_t1 = __builtin_amdgcn_s_memrealtime();
#endif
            for (int spin = 0; spin < TR_SPIN_LIMIT; ++spin) {
                hw = __hip_atomic_load(&hand[wv + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                f = (UNI((unsigned)(hw >> 42)) == ttag) ? (int)(UNI((unsigned)(hw >> 40)) & 3u) : 0;
                if (f) break;
                __builtin_amdgcn_s_sleep(2);
            }
            if (f != 1) { err = 5; break; }                 // the chunk above failed (or timed out)
#ifdef PWR_DIAG
            tr_t2 = __builtin_amdgcn_s_memrealtime();
#endif
            y = (int)(UNI((unsigned)hw) & 0xffffffu) - 1;
            if (y == yguess && xrec_lo <= x_lo) break;      // the guess was right and the whole chunk is recorded
            check_merge = true;
        }
        int gcur = -1, yb = 0;
        uint32_t win[4] = {0, 0, 0, 0};
        int gpre = -1, ybpre = 0;
        uint32_t pre[4] = {0, 0, 0, 0};
        int blk = x >> 6;
        int wcur = way[min(blk * 64 + lane, L - 1)];
        int wnxt = way[max(blk * 64 - 64 + lane, 0)];
        int ncreg = 0, yireg = 0;
        if (phase == 1) { ncreg = newcol[min(blk * 64 + lane, L - 1)]; yireg = yin[min(blk * 64 + lane, L - 1)]; }
        bool merged = false;
        while (x >= x_lo && !err) {
            x = UNI(x); y = UNI(y); blk = UNI(blk); gcur = UNI(gcur); yb = UNI(yb); gpre = UNI(gpre); ybpre = UNI(ybpre); cnt = UNI(cnt);
            if (phase == 0) {
                // ---- fast path (phase 0 only): rows of the current 16-row group / 64-row block whose answer
                //      lies in the 64-cell sub-window holding the current column
                while ((x >> 4) == gcur && (x >> 6) == blk && x >= x_lo) {
                    const int af = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
                    const int ycf = min(y, af + min(B, W - af) - 1);
                    if (y < af || ycf < yb || ycf > yb + 255) break;
                    const int q0 = (ycf - yb) >> 6, shf = 15 - (x & 15);
                    const uint32_t wq = q0 == 0 ? win[0] : q0 == 1 ? win[1] : q0 == 2 ? win[2] : win[3];
                    const int cy = yb + 64 * q0 + lane;
                    const unsigned long long mk = __ballot(cy <= ycf && cy >= af && !((wq >> shf) & 1u));
                    if (!mk) break;
                    const int t = 63 - __builtin_clzll(mk);
                    const int yy = yb + 64 * q0 + t;
                    const int cb = (int)((__ballot((wq >> (16 + shf)) & 1u) >> t) & 1ull);
                    ncreg = (lane == (x & 63)) ? ((yy << 1) | (cb ^ 1)) : ncreg;
                    yireg = (lane == (x & 63)) ? y : yireg;
                    y = yy - cb;                            // diag: column to the left, up: stay
                    cnt += cb ^ 1;
                    --x;
                    if (y < 0) break;
                }
                if (x < x_lo) break;
                if (y < 0) { err = 3; break; }
            }
            if ((x >> 6) != blk) {
                if (blk * 64 + lane < L) { newcol[blk * 64 + lane] = ncreg; yin[blk * 64 + lane] = yireg; }
                blk = x >> 6;
                wcur = wnxt;
                wnxt = way[max(blk * 64 - 64 + lane, 0)];
                if (phase == 1) { ncreg = newcol[min(blk * 64 + lane, L - 1)]; yireg = yin[min(blk * 64 + lane, L - 1)]; }
            }
            if (check_merge && x >= xrec_lo && __builtin_amdgcn_readlane(yireg, x & 63) == y) { merged = true; break; }
            const int a = max(0, __builtin_amdgcn_readlane(wcur, x & 63) - H);
            const int Bx = min(B, W - a);
            if (y < a) { err = 1; break; }
            int yc = min(y, a + Bx - 1);                     // past the band: implicit left moves
            const int g = x >> 4, sh = 15 - (x & 15);
            int found = -1, cbit = 0;
            for (;;) {
                if (g != gcur || yc < yb || yc > yb + 255) {
                    const int want = max(lo, yc - 191);
                    if (gpre == g && ybpre == want) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) win[q] = pre[q];
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) win[q] = dirs[(size_t)g * RS + (want + 64 * q + lane - lo) % RS];
                    }
                    gcur = g; yb = want;
                    if (g > 0) {
                        gpre = g - 1; ybpre = want;
#pragma unroll
                        for (int q = 0; q < 4; ++q) pre[q] = dirs[(size_t)(g - 1) * RS + (want + 64 * q + lane - lo) % RS];
                    }
                }
                {
                    const int q0 = (yc - yb) >> 6;
                    const uint32_t wq = q0 == 0 ? win[0] : q0 == 1 ? win[1] : q0 == 2 ? win[2] : win[3];
                    const int cy = yb + 64 * q0 + lane;
                    const unsigned long long mk = __ballot(cy <= yc && cy >= a && !((wq >> sh) & 1u));
                    if (mk) {
                        const int t = 63 - __builtin_clzll(mk);
                        found = yb + 64 * q0 + t;
                        const unsigned long long ck = __ballot((wq >> (16 + sh)) & 1u);
                        cbit = (int)((ck >> t) & 1ull);
                    } else {
#pragma unroll
                        for (int q = 2; q >= 0; --q) {
                            if (found < 0 && q < q0) {
                                const int cy2 = yb + 64 * q + lane;
                                const unsigned long long mk2 = __ballot(cy2 >= a && !((win[q] >> sh) & 1u));
                                if (mk2) {
                                    const int t = 63 - __builtin_clzll(mk2);
                                    found = yb + 64 * q + t;
                                    const unsigned long long ck = __ballot((win[q] >> (16 + sh)) & 1u);
                                    cbit = (int)((ck >> t) & 1ull);
                                }
                            }
                        }
                    }
                }
                if (found >= 0) break;
                if (yb <= a) { err = 2; break; }
                yc = yb - 1;
            }
            if (err) break;
            const int yy = found;
            const int nv = cbit ? (yy << 1) : ((yy << 1) | 1);                       // PW:1394 (c) / PW:1404 (d)
            if (phase == 1 && x >= xrec_lo) cnt -= __builtin_amdgcn_readlane(ncreg, x & 63) & 1;   // replaces a recorded step
            cnt += nv & 1;
            ncreg = (lane == (x & 63)) ? nv : ncreg;
            yireg = (lane == (x & 63)) ? y : yireg;
            y = cbit ? yy - 1 : yy;
            --x;
            if (x >= 0 && y < 0) { err = 3; break; }
        }
        if (blk * 64 + lane < L && (x < x_top)) { newcol[blk * 64 + lane] = ncreg; yin[blk * 64 + lane] = yireg; }
        if (phase == 0) {
            if (top) {
                if (err) break;
            } else {
                // a failed guess is harmless: rows x+1 .. x_top are recorded (and counted), row x is where it broke off
                xrec_lo = err ? x + 1 : x_lo;
                if (err == 0) yout_guess = y;
                err = 0;
            }
            if (top) { yout_guess = y; }
        } else {
            if (err) break;
            if (merged && xrec_lo > x_lo) { err = 6; break; }   // merged into a guess that broke off: the true trace breaks there too
            if (merged) y = yout_guess;                     // the rest of the chunk is what the guess recorded
            yout_guess = y;
        }
    }
    // a guess that broke off early leaves rows below xrec_lo unrecorded: phase 1 retraced through them (no merge
    // is possible there), so every row of the chunk is final now
    if (lane == 0)
        __hip_atomic_store(&hand[wv], TR_WORD(ttag, err ? 2 : 1, cnt, yout_guess), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (err) {
        if (lane == 0) { m->ok = 0; atomicCAS(&st.hdr->status, 0, PWR_ERR_INTERNAL); }
        return;
    }
#ifdef PWR_DIAG
    if (job == 0 && lane == 0 && (wv == 0 || top)) {
        const unsigned long long n_ = __builtin_amdgcn_s_memrealtime();
        unsigned long long *d_ = st.hdr->dbg + (top ? 20 : 16);
        d_[0] += (top ? n_ : tr_t1) - tr_t0; d_[1] += tr_t2 - tr_t1; d_[2] += n_ - (top ? n_ : tr_t2); d_[3] += 1;
    }
#endif
    if (wv == 0 && lane == 0) {
        int tot = cnt;
        for (int c = 1; c < nch; ++c)                       // all chunks above are final (hand-over order) and posted
            tot += (int)((__hip_atomic_load(&hand[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 24) & 0xffffull);
        m->nnew = tot;
        m->changed = 1;                                     // (not worked out here: the commit takes the long way)
    }
}

// ---------------------------------------------------------------------------------------------
// trace, one wave per TB_C-row block ("chunk"), hand-over without a chain.  As in k_trace_par every chunk but the top one
// first traces its rows from a GUESSED arrival column (just left of where the row above sits now) and records, per row,
// the arrival column and the placement; it then posts a word {arrival column it started from, exit column, 'up' moves}.
// What k_trace_par resolves top-down, one chunk after the other (a chain of L / 192 hand-overs, a third of its time), every
// chunk settles here for itself, from the words of the chunks above it:
//   * whenever the exit the chunk above posts differs from the arrival a chunk has traced from, it retraces from there
//     (until it arrives at a recorded row in the column the record arrived in: the recorded steps below are then the true
//     ones) and posts again -- all chunks whose guess was wrong do that at the same time, each trusting the exit above it;
//   * a chunk is FINAL once the chunks above it form a consistent chain -- each one's arrival equal to the exit posted by
//     the chunk above it -- up to a chunk that is final (the top chunk is, from the start: it begins in the entry column).
//     A step of the trace is a function of (row, column), so a record traced from the true arrival is the true record,
//     whatever else its chunk may post later; by induction down the chain every exit in it is the true one.
// A chunk only ever waits for a chunk above it, and retraces only when an exit above it has changed, which ends with the top
// chunk's.  Results are those of k_trace_wp bit for bit.
// word: [63:50] launch tag, [49:48] 1 provisional / 2 final / 3 error, [47:41] 'up' moves, [40:21] arrival + 1, [20:0] exit + 1
// (exit field all ones: the pass broke off inside the chunk)
// ---------------------------------------------------------------------------------------------
#define TB_W 4                                          // chunks per work-group
#ifndef TB_C
#define TB_C 32                                         // rows per chunk (one lane per row; a row of the trace costs ~290 ns of dependent
                                                        // instructions, so a chunk half as long is traced in half the time: 64 -> 32 rows, 30 -> 20 us)
#endif
#define TB_BROKE 0x1fffffu
#define TBP_LOOK 8                                      // columns a row's prior looks at: Way[x] .. Way[x] + 7 (rows sit ~4.5 columns apart)
#define TB_WORD(TAG, FLAG, CNT, ARR, EXF) (((unsigned long long)((TAG) & 0x3fffu) << 50) | ((unsigned long long)(FLAG) << 48) | ((unsigned long long)((CNT) & 0x7f) << 41) | \
                                           ((unsigned long long)(((ARR) + 1) & 0xfffff) << 21) | (unsigned long long)((EXF) & 0x1fffffu))
#define TB_MAXCOL ((1 << 20) - 4)                       // columns the word can name
__global__ __launch_bounds__(TB_W * 64) void k_trace_blk(DState st, JobBufs jb)
{
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    // The check of the segments' starts rides in this launch (`check_in_trace`): its work-groups come behind the traceback's and
    // run beside them -- a launch less per batch (5.6 us + a kernel boundary).  The traceback therefore starts without the
    // verdict: a job whose check fails is traced like any other (its record is that of a DP from other starts: well-formed,
    // only not the true one), nobody uses the result (k_commit_scan looks at the verdict), and the one thing that must not
    // happen -- an inconsistent record of such a job reported as an error -- waits for the verdict first (below).
    if (jb.check_in_trace && (int)blockIdx.y >= jb.trace_ny) { seg_check_body(st, jb, job, (int)blockIdx.y - jb.trace_ny + 1, tid); return; }
    JobMeta *m = &jb.meta[job];
    const int L = UNI(m->L);
    if (!m->active || L <= 0 || !m->ok || m->abort || (!jb.check_in_trace && m->segfail) || (m->wide && !jb.f64_follows) || NOT_MINE(jb, job)) return;   // (not filled: stalled, failed its check, or its batch came without k_fill64)
    const int nch = (L + TB_C - 1) / TB_C;
    // the top chunks first: they are the ones everybody else waits for
    const int c = nch - 1 - UNI((int)blockIdx.y * TB_W + (tid >> 6));
    if (c < 0) return;
    unsigned long long *const hand = jb.gtr + (size_t)job * jb.trk;
    const unsigned ttag = jb.trace_tag & 0x3fffu;
    const int W = UNI(m->W), B = st.B, H = st.H, RS = jb.NC, lo = UNI(m->lo);
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const uint32_t *dirs = jb.dirs + (size_t)job * jb.dirstride;
    const unsigned *lastM = jb.lastM + (size_t)job * jb.NC;
    int *newcol = jb.newcol + (size_t)job * jb.Lmax;
    int *yin = jb.aux + (size_t)job * jb.Lmax;             // arrival column per row (aux is rewritten by the commit later)
    const int x_lo = c * TB_C, x_top = min(L, x_lo + TB_C) - 1;
    const bool top = c == nch - 1;
    const int wcur = way[min(x_lo + lane, L - 1)];         // Way[] of the chunk's rows, one per lane
    int ncreg = 0, yireg = 0;                              // the chunk's record, one row per lane
    int xrec_lo = x_top + 1;                               // rows [xrec_lo, x_top] are recorded
    int cnt = 0, err = 0, yexit = 0;
    bool broke = false;                                    // the last pass from the top of the chunk did not reach its bottom

    // The prior (`trace_prior`): a realignment leaves most bases where they are.  For row x < L - 1 the present
    // placement says: arrive in column Way[x+1] - 1, step to Way[x] by a diagonal move, leave in Way[x] - 1.  A step of the
    // trace is a function of (row, column), so whether the record agrees is a property of the row alone: applied at
    // (x, Way[x+1] - 1) the step below finds Way[x] iff, after the band clamp, the A bit is set in every column of
    // (Way[x], ycf] and clear in Way[x], and it is a diagonal one iff the C bit is set there.  One row per lane, the words of
    // a row's columns all in flight at once; a gap of more than TBP_LOOK columns, an arrival left of the band, anything else
    // that does not fit: "not intact", and the row is stepped as ever.  A pass that arrives at an intact row in that very
    // column records the whole run of intact rows below it in one assignment and goes on under the run.  (The test of a step
    // against the prior is on the chain of every row that is NOT intact: one v_readlane of `ppri` and a compare.)
    const int wnx = __shfl_down(wcur, 1);                  // Way[x+1] (lane TB_C - 1: the bottom row of the chunk above; lane 63 gets its own Way: never intact)
    unsigned long long pmask = 0ull;                       // bit l: row x_lo + l is intact
    int ppri = -2;                                         // ... and the column its prior arrives in (-2: not intact; an arrival is >= -1)
    if (jb.trace_prior) {
        const int xr = x_lo + lane, ya = wnx - 1;
        const int af = max(0, wcur - H);
        const int ycf = min(ya, af + min(B, W - af) - 1);
        // (a run ends in a row that leaves in a column >= 0 or is row 0: no way into the 'y < 0' error from inside one)
        bool ok = lane < TB_C && xr < L - 1 && ya >= af && ycf >= wcur && ycf - wcur < TBP_LOOK && wcur >= lo && RS >= TBP_LOOK && (wcur >= 1 || xr == 0);
        const int i0 = ok ? (wcur - lo) % RS : 0, span = ok ? ycf - wcur : -1;
        const uint32_t *drow = dirs + (size_t)(min(xr, L - 1) >> 4) * RS;
        uint32_t pw[TBP_LOOK];
#pragma unroll
        for (int k = 0; k < TBP_LOOK; ++k) { const int i = i0 + k; pw[k] = k <= span ? drow[i >= RS ? i - RS : i] : 0u; }
        const int sh = 15 - (xr & 15);
        ok = ok && ((pw[0] >> sh) & 0x10001u) == 0x10000u;                      // A clear, C diag in Way[x]
#pragma unroll
        for (int k = 1; k < TBP_LOOK; ++k) ok = ok && (k > span || ((pw[k] >> sh) & 1u));
        pmask = __ballot(ok);
        ppri = ok ? ya : -2;
    }
    const bool prior = UNI(jb.trace_prior) != 0;
    // 'up' moves among the recorded rows: what the chunk's word carries
    auto ups = [&]() __attribute__((always_inline)) {
        return (int)__builtin_popcountll(__ballot(lane < TB_C && x_lo + lane >= xrec_lo && x_lo + lane <= x_top && (ncreg & 1)));
    };

    // one pass over the chunk's rows from arrival column y0: records as it goes; with check_merge it stops as soon as it
    // arrives at a recorded row in the column the record arrived in (the recorded steps below are then the true ones)
    // (PRIOR: std::true_type / std::false_type -- without the prior the pass is the one of round 6, instruction for instruction)
    auto pass_t = [&](auto PRIOR, int y0, const bool check_merge, bool &merged) __attribute__((always_inline)) {
        int x = x_top, y = y0;
        int gcur = -1, yb = 0;
        uint32_t win[4] = {0, 0, 0, 0};
        int gpre = -1, ybpre = 0;
        uint32_t pre[4] = {0, 0, 0, 0};
        merged = false;
        int e = 0;
        // at (x, y): row x is intact and y is the column its prior arrives in -> record the run of intact rows that ends in x
        auto take_run = [&]() __attribute__((always_inline)) {
            if constexpr (!decltype(PRIOR)::value) return false;
            const int l = x & (TB_C - 1);
            if (__builtin_amdgcn_readlane(ppri, l) != y) return false;
            const unsigned long long inv = ~pmask & ((2ull << l) - 1ull);
            const int l0 = inv ? 64 - __builtin_clzll(inv) : 0;                // the lowest row of the run
            const bool in = lane >= l0 && lane <= l;
            ncreg = in ? (wcur << 1) : ncreg;
            yireg = in ? wnx - 1 : yireg;
            y = __builtin_amdgcn_readlane(wcur, l0) - 1;
            x = x_lo + l0 - 1;
            return true;
        };
        while (x >= x_lo && !e) {
            x = UNI(x); y = UNI(y); gcur = UNI(gcur); yb = UNI(yb); gpre = UNI(gpre); ybpre = UNI(ybpre);
            // ---- the common case, straight: rows of the current 16-row group whose step lies in the 64-cell part of the window
            //      that holds the current column
            while ((x >> 4) == gcur && x >= x_lo) {
                if (check_merge && x >= xrec_lo && __builtin_amdgcn_readlane(yireg, x & (TB_C - 1)) == y) { merged = true; break; }
                if (take_run()) continue;
                const int af = max(0, __builtin_amdgcn_readlane(wcur, x & (TB_C - 1)) - H);
                const int ycf = min(y, af + min(B, W - af) - 1);
                if (y < af || ycf < yb || ycf > yb + 255) break;
                const int q0 = (ycf - yb) >> 6, shf = 15 - (x & 15);
                const uint32_t wq = q0 == 0 ? win[0] : q0 == 1 ? win[1] : q0 == 2 ? win[2] : win[3];
                const int cy = yb + 64 * q0 + lane;
                const unsigned long long mk = __ballot(cy <= ycf && cy >= af && !((wq >> shf) & 1u));
                if (!mk) break;
                const int t = 63 - __builtin_clzll(mk);
                const int yy = yb + 64 * q0 + t;
                const int cb = (int)((__ballot((wq >> (16 + shf)) & 1u) >> t) & 1ull);
                const int nv = (yy << 1) | (cb ^ 1);                               // PW:1394 (c) / PW:1404 (d)
                ncreg = (lane == (x & (TB_C - 1))) ? nv : ncreg;
                yireg = (lane == (x & (TB_C - 1))) ? y : yireg;
                y = yy - cb;                                                       // diag: column to the left, up: stay
                --x;
                if (x >= 0 && y < 0) { e = 3; break; }
            }
            if (merged || e || x < x_lo) break;
            if (check_merge && x >= xrec_lo && __builtin_amdgcn_readlane(yireg, x & (TB_C - 1)) == y) { merged = true; break; }
            if (take_run()) continue;
            const int a = max(0, __builtin_amdgcn_readlane(wcur, x & (TB_C - 1)) - H);
            const int Bx = min(B, W - a);
            if (y < a) { e = 1; break; }
            int yc = min(y, a + Bx - 1);                     // past the band: implicit left moves
            const int g = x >> 4, sh = 15 - (x & 15);
            int found = -1, cbit = 0;
            for (;;) {
                if (g != gcur || yc < yb || yc > yb + 255) {
                    // the window of the group above was fetched ahead for this group as well, a little to the left: take it
                    // if the column still lies in its right part (room for the steps to the left that are to come)
                    if (gpre == g && yc >= ybpre + 96 && yc <= ybpre + 255) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) win[q] = pre[q];
                        yb = ybpre;
                    } else {
                        const int want = max(lo, yc - 191);
#pragma unroll
                        for (int q = 0; q < 4; ++q) win[q] = dirs[(size_t)g * RS + (want + 64 * q + lane - lo) % RS];
                        yb = want;
                    }
                    gcur = g;
                    if (g > (x_lo >> 4)) {
                        gpre = g - 1; ybpre = max(lo, yb - 56);      // a trace drifts left by about 4.5 columns per row
#pragma unroll
                        for (int q = 0; q < 4; ++q) pre[q] = dirs[(size_t)(g - 1) * RS + (ybpre + 64 * q + lane - lo) % RS];
                    }
                }
                {
                    const int q0 = (yc - yb) >> 6;
                    const uint32_t wq = q0 == 0 ? win[0] : q0 == 1 ? win[1] : q0 == 2 ? win[2] : win[3];
                    const int cy = yb + 64 * q0 + lane;
                    const unsigned long long mk = __ballot(cy <= yc && cy >= a && !((wq >> sh) & 1u));
                    if (mk) {
                        const int t = 63 - __builtin_clzll(mk);
                        found = yb + 64 * q0 + t;
                        const unsigned long long ck = __ballot((wq >> (16 + sh)) & 1u);
                        cbit = (int)((ck >> t) & 1ull);
                    } else {
#pragma unroll
                        for (int q = 2; q >= 0; --q) {
                            if (found < 0 && q < q0) {
                                const int cy2 = yb + 64 * q + lane;
                                const unsigned long long mk2 = __ballot(cy2 >= a && !((win[q] >> sh) & 1u));
                                if (mk2) {
                                    const int t = 63 - __builtin_clzll(mk2);
                                    found = yb + 64 * q + t;
                                    const unsigned long long ck = __ballot((win[q] >> (16 + sh)) & 1u);
                                    cbit = (int)((ck >> t) & 1ull);
                                }
                            }
                        }
                    }
                }
                if (found >= 0) break;
                if (yb <= a) { e = 2; break; }
                yc = yb - 1;
            }
            if (e) break;
            const int yy = found;
            const int nv = cbit ? (yy << 1) : ((yy << 1) | 1);                       // PW:1394 (c) / PW:1404 (d)
            ncreg = (lane == (x & (TB_C - 1))) ? nv : ncreg;
            yireg = (lane == (x & (TB_C - 1))) ? y : yireg;
            y = cbit ? yy - 1 : yy;
            --x;
            if (x >= 0 && y < 0) { e = 3; break; }
        }
        // rows above x are recorded now (a pass that broke off leaves the rows below as they were)
        if (!merged) xrec_lo = e ? min(xrec_lo, x + 1) : x_lo;
        if (!e && !merged) yexit = y;
        return e;
    };
    auto pass = [&](int y0, const bool check_merge, bool &merged) __attribute__((always_inline)) {
        return prior ? pass_t(std::true_type{}, y0, check_merge, merged) : pass_t(std::false_type{}, y0, check_merge, merged);
    };
#define TB_POST(FLAG, ARR) cnt = ups(); if (lane == 0) __hip_atomic_store(&hand[c], TB_WORD(ttag, FLAG, cnt, ARR, broke ? TB_BROKE : (unsigned)(yexit + 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    bool merged = false;
#ifdef PWR_DIAG
    const unsigned long long tb_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long tb_t1 = tb_t0;
    int tb_looks = 0, tb_retr = 0;
#endif
    if (top) {
        // entry: minimum of the last row over y in [ylow, W-1], ties -> largest y; columns past the band carry the value of
        // the last band cell (PW:287)
        const int wx = UNI(way[L - 1]);
        const int a = max(0, wx - H), Bx = min(B, W - a);
        int ylow = max(-1, wx - H) + 1;
        if (ylow > W - 1) ylow = W - 1;
        unsigned long long key = ~0ull;
        {
            // (every chunk waits for this one: the scores are fetched in one go -- a loop that loads, compares and loads again pays a
            // memory round trip per 64 columns, 4 us of the launch's 24 at a bandwidth of 1000)
            constexpr int EN = (PWR_MAX_BANDWIDTH + 63) / 64;
            const int y0_ = max(ylow, a) + lane;
            unsigned ev[EN];
#pragma unroll
            for (int i = 0; i < EN; ++i) { const int yy = y0_ + 64 * i; ev[i] = yy < a + Bx ? lastM[(yy - lo) % RS] : 0xffffffffu; }
#pragma unroll
            for (int i = 0; i < EN; ++i) {
                const int yy = y0_ + 64 * i;
                const unsigned long long k2 = yy < a + Bx ? (((unsigned long long)ev[i] << 32) | (unsigned)(~(unsigned)yy)) : ~0ull;
                key = k2 < key ? k2 : key;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o);
            key = other < key ? other : key;
        }
        const unsigned vmin = (unsigned)(key >> 32);
        int entry = (key == ~0ull) ? -1 : (int)(~(unsigned)key);
        if (a + B <= W - 1) {
            const unsigned lastval = lastM[(a + B - 1 - lo) % RS];
            if (entry < 0 || lastval <= vmin) entry = W - 1;
        }
        entry = UNI(entry);
        if (lane == 0) m->entry = entry;
        err = entry < 0 ? 4 : pass(entry, false, merged);
    } else {
        int arr = UNI(way[x_top + 1]) - 1;                         // the guess
        broke = pass(arr, false, merged) != 0;                     // (a guess that breaks off is harmless: the rows above the break are recorded)
        TB_POST(1, arr)
#ifdef PWR_DIAG
        tb_t1 = __builtin_amdgcn_s_memrealtime();
#endif
        for (int look = 0; look < (1 << 16) && !err; ++look) {
#ifdef PWR_DIAG
            tb_looks += 1;
#endif
            int t = c + 1;                                     // chunks [c + 1, t) are consistent so far
            int verdict = 0;                                   // 1: the chain above closes at a final chunk, 2: chunk `bad` is not settled
            int bad = -1;
            unsigned long long wbad = 0;
            unsigned ex_first = 0;                             // exit field of chunk c + 1
            while (!verdict && !err) {
                // words of the chunks t .. t + 63, and of t + 64 for the last lane's comparison
                const int j = min(t + lane, nch - 1);
                unsigned long long w = 0, wn = 0;
                int st_j = 0;
                for (int spin = 0; spin < TR_SPIN_LIMIT; ++spin) {
                    w = __hip_atomic_load(&hand[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    st_j = ((unsigned)(w >> 50) == ttag) ? (int)((w >> 48) & 3ull) : 0;
                    if (__ballot(st_j == 0) == 0ull) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (__ballot(st_j == 0) != 0ull || __ballot(st_j == 3) != 0ull) { err = 5; break; }
                const unsigned ex_j = (unsigned)w & 0x1fffffu, ar_j = (unsigned)(w >> 21) & 0xfffffu;
                unsigned ex_up = (unsigned)__shfl_down((int)ex_j, 1);               // exit of the chunk above chunk j
                if (lane == 63) {
                    const int j2 = min(t + 64, nch - 1);
                    int s2 = 0;
                    for (int spin = 0; spin < TR_SPIN_LIMIT; ++spin) {
                        wn = __hip_atomic_load(&hand[j2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s2 = ((unsigned)(wn >> 50) == ttag) ? (int)((wn >> 48) & 3ull) : 0;
                        if (s2) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                    ex_up = s2 == 0 || s2 == 3 ? 0u : ((unsigned)wn & 0x1fffffu);
                }
                const bool valid = t + lane <= nch - 1;
                const bool fin = valid && st_j == 2;
                const bool cons = valid && (st_j == 2 || (t + lane < nch - 1 && ar_j == ex_up));   // (arrival + 1 == exit + 1)
                if (t == c + 1) ex_first = (unsigned)__builtin_amdgcn_readlane((int)ex_j, 0);
                const unsigned long long mfin = __ballot(fin), mbad = __ballot(valid && !cons);
                const int ffin = mfin ? __builtin_ctzll(mfin) : 64, fbad = mbad ? __builtin_ctzll(mbad) : 64;
                if (ffin < 64 && ffin <= fbad) verdict = 1;
                else if (fbad < 64) {
                    verdict = 2; bad = t + fbad;
                    wbad = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(w >> 32), fbad) << 32) | (unsigned)__builtin_amdgcn_readlane((int)w, fbad);
                }
                else t += 64;                                  // 64 more consistent chunks: look further up
            }
            if (err) break;
            if (ex_first == TB_BROKE) {
                // the record of the chunk above breaks off: if that is its true record, the trace itself is inconsistent
                if (verdict == 1) { err = 6; break; }
            } else if ((int)ex_first - 1 != arr) {
                // the chunk above leaves in another column than this one started from: trace again from there, at once (its
                // exit is usually what it will stay; if not, this happens again)
                arr = (int)ex_first - 1;
#ifdef PWR_DIAG
                tb_retr += 1;
#endif
                const int e1 = pass(arr, true, merged);
                if (e1) broke = true;
                else if (merged) { if (xrec_lo > x_lo) broke = true; }    // merged into a record that breaks off further down
                else broke = false;
                TB_POST(1, arr)
                continue;
            } else if (verdict == 1) break;                    // traced from the true arrival: final
            // something above is not settled yet: look again when that chunk has posted anew
            for (int spin = 0; spin < TR_SPIN_LIMIT; ++spin) {
                const unsigned long long w = __hip_atomic_load(&hand[bad], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (UNI((unsigned)w) != (unsigned)wbad || UNI((unsigned)(w >> 32)) != (unsigned)(wbad >> 32)) break;
                if (spin == TR_SPIN_LIMIT - 1) { err = 5; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (!err && broke) err = 6;                               // the true trace breaks off in this chunk
        if (!err) { TB_POST(2, arr) }
    }
    if (lane < TB_C && x_lo + lane < L) { newcol[x_lo + lane] = ncreg; yin[x_lo + lane] = yireg; }
    // did any base of the chunk move (or open a column)?  If none of the row's does, its commit has nothing to do.
    if (__ballot(lane < TB_C && x_lo + lane < L && ncreg != (wcur << 1)) != 0ull && lane == 0) __hip_atomic_store(&m->changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (top || err) {
        cnt = ups();
        if (lane == 0)
            __hip_atomic_store(&hand[c], TB_WORD(ttag, err ? 3 : 2, cnt, 0, (unsigned)(yexit + 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef PWR_DIAG
    if (job == 0 && lane == 0) {
        const unsigned long long n_ = __builtin_amdgcn_s_memrealtime();
        if (tb_retr) atomicAdd(&st.hdr->dbg[24], (unsigned long long)tb_retr);   // retraces
        if (c == 0 || top) {
            unsigned long long *d_ = st.hdr->dbg + (top ? 20 : 16);
            d_[0] += (top ? n_ : tb_t1) - tb_t0; d_[1] += n_ - (top ? n_ : tb_t1); d_[3] += 1;
            if (c == 0) { st.hdr->dbg[25] += (unsigned long long)tb_looks; st.hdr->dbg[26] += (unsigned long long)nch; }
        }
    }
#endif
    if (err) {
        if (lane == 0) {
            bool failed = false;
            if (jb.check_in_trace && seg_check_applies(st, jb, job, m)) {
                // the record of a job whose check failed may be anything: wait for the verdict (its work-groups are in this launch,
                // a few microseconds of work each; bounded all the same)
                const int want = m->nseg - 1;
                for (unsigned spin = 0; spin < (1u << 22) && __hip_atomic_load(&jb.chkdone[job], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want; ++spin) __builtin_amdgcn_s_sleep(8);
                failed = __hip_atomic_load(&m->segfail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
            }
            if (!failed) { m->ok = 0; atomicCAS(&st.hdr->status, 0, PWR_ERR_INTERNAL); }
        }
        return;
    }
    if (c == 0) {
        // every chunk above is final, or its latest word is of a record traced from the true arrival: their 'up' moves add up
        // to the columns this realignment opens
        int tot = 0;
        for (int j = lane; j < nch; j += 64)
            tot += (int)((__hip_atomic_load(&hand[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 41) & 0x7full);
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        if (lane == 0) m->nnew = tot;
    }
#undef TB_POST
}

// ---------------------------------------------------------------------------------------------
// commit: Column_Updater (PW:1222-1243) for every existing column a realigned row touches, Column_Adder (PW:1245-1332) for
// every column it opens, then W_Con (PW:706-763): drop the columns without a base and renumber -- for ALL the jobs of a batch
// that may commit, spread over the chip in two launches (round 3: one work-group that walked the jobs one after the other,
// 68 us per batch; a kernel boundary costs less than a grid barrier inside a launch, so a phase that needs every work-group
// of the one before is a launch -- and only such a phase):
//   k_commit_scan    (job, share): WHAT a job's new placement changes, without touching the state: the columns whose symbol for
//                    the row changes, the columns it opens (with their AlGapCount, PW:1305-1314 = coverage - rows ending there,
//                    both without the row) and the columns it empties -- and which of that lies in the band interval of a LATER
//                    job of the batch (the jobs of a batch are all gathered from the same state, in the same numbering);
//   k_commit_finish  decides which jobs commit -- in row order; a job is exact iff no job committed before it changes anything
//                    inside its interval [lo, hi] (every column its DP read) and the clamps at the MSA's edges see the same
//                    distances (PW:1496-1497, 1505); a job may go AHEAD of a stale one when their intervals are disjoint --,
//                    applies the changes of all of them (their column sets are disjoint by that very rule), writes the order
//                    under its new ordinals, new columns included, into the OTHER order buffer, and the last work-group to
//                    arrive frees the emptied columns and writes the header: width, which buffer is current, row pointer, the
//                    next batch's size, the copy for the host.
// The changes and the renumbering were a launch each while the renumbering worked in place (source and target ranges of the
// stretches that move overlap across work-groups).  Nothing else the renumbering reads comes from another work-group: the plan
// and the sorted events every work-group works out for itself, and a new column's slot (aux[x]) is written and read by the same
// thread.  The last arriver's ticket is the only synchronisation between the work-groups of the commit.
// ---------------------------------------------------------------------------------------------
#define COMMIT_NT 1024
#define EVCAP 1024                  // structural events (columns opened / emptied) of one BATCH handled without a pass over the width
#define MAXJ 128                    // jobs of a batch ("window" <= 128)
#define CS_G 16                     // shares of a job in k_commit_scan
#define CA_G 32                     // work-groups of k_commit_finish

// symbol of the realigned row in existing column y: base+? from a mark array inside [y0,y1], blank outside
__device__ __forceinline__ int row_symbol(const uint8_t *mk, int y, int lo, int y0, int y1)
{
    if (y < y0 || y > y1) return 5;
    const int v = mk[y - lo];
    return v == 7 ? 5 : (v ? v - 1 : 4);                  // 7: a blank run between two segments of the row
}

enum { V_NONE = 0, V_COMMIT, V_STALE, V_STOP_NOTOK, V_STOP_GROW, V_STOP_WIDE, V_STOP_ABORT, V_STOP_SEGFAIL, V_EMPTY, V_AFTER_STOP };
struct BatchPlan {
    int idle;                       // sticky error or capacity shortage: the batch does nothing
    int ncommit, nnew, ndel, nev;   // jobs that commit; columns they open / empty; their structural events
    int restructure, big;           // the order changes; ... by a pass over the width (more than evcap events)
    int live_all, live_done, ahead_n;
    int first;                      // first ordinal that changes
    unsigned long long done_mask;
    int reasons[4];
    int cjobs[MAXJ], slotbase[MAXJ];          // the committing jobs in row order; index of a job's first new column among the batch's
    signed char verdict[MAXJ];
};
struct CommitEv { int key[EVCAP], dl[EVCAP], skey[EVCAP], scum[EVCAP], del[EVCAP]; int cum, nev, ndel, pad; };   // (in LDS, one per work-group)

__global__ __launch_bounds__(COMMIT_NT) void k_commit_scan(DState st, JobBufs jb, int njobs)
{
    __shared__ unsigned sh[COMMIT_NT / 64];
    constexpr int CPQ = (PWR_MAX_SEQ_LENGTH / TB_C + COMMIT_NT) / COMMIT_NT;   // chunks of the traceback per thread of the prefix below
    __shared__ int s_cpre[COMMIT_NT * CPQ];
    __shared__ int s_ov[MAXJ], s_ovlo[MAXJ], s_ovhi[MAXJ], s_nov;
    const int job = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const JobMeta *m = &jb.meta[job];
    if (st.hdr->status != 0 || st.hdr->need_grow) return;
    if (!m->active || m->L <= 0 || !m->ok || m->abort || m->segfail || (m->wide && !jb.f64_follows)) return;   // cannot commit in this batch
    const int k = m->k, L = m->L;
    if (!m->changed && st.nbrk[k] == 0) return;           // the traceback left every base where it was (k_trace_blk): nothing changes
    const int nch = (L + TB_C - 1) / TB_C;
    const bool chunked = jb.trace_blk != 0 && nch <= COMMIT_NT * CPQ;   // k_trace_blk counted the 'up' moves of every TB_C rows
    const int G = (chunked && L >= 64 * CS_G) ? CS_G : 1;
    if (g >= G) return;
    CommitJob *cj = &jb.cjob[job];
    const long long off = st.rowoff[k];
    const int lo = m->lo;
    const int *order = cur_order(st);
    const int *way = jb.way + (size_t)job * jb.Lmax;
    const int *newcol = jb.newcol + (size_t)job * jb.Lmax;
    int *aux = jb.aux + (size_t)job * jb.Lmax;
    int *insidx = jb.insidx + (size_t)job * jb.Lmax;
    const uint8_t *mark = jb.mark + (size_t)job * jb.colcap;
    uint8_t *mark2 = jb.mark2 + (size_t)job * jb.colcap;
    int *list = jb.chg + (size_t)job * jb.colcap;
    int *evkey = jb.evkey + (size_t)job * EVCAP, *evdl = jb.evdl + (size_t)job * EVCAP;
    const int way0 = way[0], wayL = way[L - 1];
    const int nc0 = newcol[0], ncL = newcol[L - 1];
    const int ny0 = (nc0 >> 1) + (nc0 & 1), nyL = ncL >> 1;   // existing columns inside the new row extent
    const int u0 = min(way0, ny0), u1 = max(wayL, nyL);
    // A share takes the bases [x0, x1) and the columns from its first base's place up to the next share's: the marks of the new
    // placement in those columns are written by its own bases only, so nothing is handed over between the shares.
    const int x0 = G == 1 ? 0 : (int)(((long long)L * g / G) & ~63LL);
    const int x1 = (G == 1 || g == G - 1) ? L : (int)(((long long)L * (g + 1) / G) & ~63LL);
    auto colpos = [](int c) { return (c >> 1) + (c & 1); };     // the first existing column at or right of a base's place
    const int Y0 = g == 0 ? u0 : colpos(newcol[x0]), Y1 = g == G - 1 ? u1 + 1 : colpos(newcol[x1]);
    if (tid == 0) {
        // the later jobs of the batch whose interval comes near this job's columns: only they can be touched
        int n = 0;
        for (int j = job + 1; j < njobs; ++j) {
            const JobMeta *mj = &jb.meta[j];
            if (!mj->active) break;
            if (mj->L <= 0) continue;
            if (mj->lo - 2 <= u1 + 2 && mj->hi + 2 >= u0 - 2) { s_ov[n] = j; s_ovlo[n] = mj->lo; s_ovhi[n] = mj->hi; ++n; }
        }
        s_nov = n;
        if (g == 0) { cj->u0 = u0; cj->u1 = u1; cj->scanned = 1; }
    }
    for (int y = Y0 + tid; y < Y1; y += COMMIT_NT) mark2[y - lo] = 0;
    if (chunked) {
        const unsigned long long *hand = jb.gtr + (size_t)job * jb.trk;
        unsigned cq[CPQ], mine = 0;
#pragma unroll
        for (int q = 0; q < CPQ; ++q) { const int ch = tid * CPQ + q; cq[q] = ch < nch ? (unsigned)((hand[ch] >> 41) & 0x7full) : 0u; mine += cq[q]; }
        unsigned tot;
        const unsigned incl = block_incl_add<COMMIT_NT>(mine, sh, tot);
        unsigned run = incl - mine;
#pragma unroll
        for (int q = 0; q < CPQ; ++q) { s_cpre[tid * CPQ + q] = (int)run; run += cq[q]; }
    }
    __syncthreads();
    const int nov = s_nov;
    // a change in column y (dl != 0: a column opens after y / column y is emptied) against the intervals of the later jobs
    auto touch = [&](int y, int dl) {
        for (int t = 0; t < nov; ++t) {
            if (y >= s_ovlo[t] - 1 && y <= s_ovhi[t] + 1) jb.pair_cf[(size_t)job * njobs + s_ov[t]] = 1;
            else if (dl != 0 && y < s_ovlo[t] - 1) atomicAdd(&jb.pair_left[(size_t)job * njobs + s_ov[t]], dl);
        }
    };
    auto event = [&](int key, int dl) {
        const int e = atomicAdd(&cj->nev, 1);
        if (e < EVCAP) { evkey[e] = key; evdl[e] = dl; }
        atomicMin(&cj->first, key >> 1);
    };
    // 1. the bases: the marks of the new placement; for every column a base opens its AlGapCount and its number among the row's
    //    new columns.  The tallies of the neighbour column y are read as the trace saw them (the state is still the gather's):
    //    the row's old symbol taken out, the new one not yet put in.
    unsigned carry = 0;
    for (int base = x0; base < x1; base += COMMIT_NT) {
        const int x = base + tid;
        const int c = x < x1 ? newcol[x] : 0;
        const unsigned ins = (x < x1 && (c & 1)) ? 1u : 0u;
        int idx;
        if (chunked) {
            // (the bases before it in its chunk: x0 is a multiple of 64, so a wave holds whole chunks)
            const unsigned long long bal = __ballot(ins != 0u);
            const int ln = tid & 63, l0 = ln & ~(TB_C - 1);
            idx = s_cpre[min(x, L - 1) / TB_C] + __builtin_popcountll(bal & ((1ull << ln) - 1ull) & ~((1ull << l0) - 1ull));
        } else {
            unsigned tot;
            const unsigned incl = block_incl_add<COMMIT_NT>(ins, sh, tot);
            idx = (int)(carry + incl - ins);
            carry += tot;
        }
        if (x < x1) {
            const int y = c >> 1;
            if (ins) {
                const Tally ty = st.tally[order[y]];
                // (the row itself out of both counts; between two of its segments it is blank, and a segment's last column
                // counts as an end -- rows read with interior blanks, until this commit)
                const bool own_nb = row_symbol(mark, y, lo, way0, wayL) != 5;
                const bool own_end = own_nb && (y == wayL || row_symbol(mark, y + 1, lo, way0, wayL) == 5);
                const uint32_t cov = ty.w[5] - (own_nb ? 1u : 0u);
                const uint32_t ends = ty.endcnt - (own_end ? 1u : 0u);
                aux[x] = (int)(cov - ends);                                        // PW:1305-1314
                insidx[x] = idx;
                event(2 * y + 1, 1);                                               // a column opens after y
                touch(y, 1);
            } else mark2[y - lo] = (uint8_t)(st.seq[off + x] + 1);
        }
    }
    __syncthreads();
    // 2. the columns: where the row's symbol changes (eight at a time: a unit inside both extents that holds the same marks
    //    before and after has none), and which of them lose their last base
    {
        const unsigned long long *mo8 = reinterpret_cast<const unsigned long long *>(mark), *mn8 = reinterpret_cast<const unsigned long long *>(mark2);
        const int ui0 = max(way0, ny0), ui1 = min(wayL, nyL);                      // columns inside both extents
        __shared__ int s_base;
        const int u_last = (Y1 - 1 - lo) >> 3;
        for (int ub = (Y0 - lo) >> 3; ub <= u_last; ub += COMMIT_NT) {
            const int u = ub + tid;
            int ent[8];
            int cnt = 0;
            if (u <= u_last) {
                const int yb8 = lo + 8 * u;
                const unsigned long long wo = mo8[u], wn = mn8[u];
                if (!(yb8 >= ui0 && yb8 + 7 <= ui1 && wo == wn)) {
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const int y = yb8 + b;
                        const int vo = (int)((wo >> (8 * b)) & 0xffull), vn = (int)((wn >> (8 * b)) & 0xffull);
                        const int so = (y < way0 || y > wayL) ? 5 : (vo == 7 ? 5 : (vo ? vo - 1 : 4));     // row_symbol()
                        const int sn = (y < ny0 || y > nyL) ? 5 : (vn == 7 ? 5 : (vn ? vn - 1 : 4));
                        // (the unit's bytes outside [Y0, Y1) are a neighbour share's)
                        const bool chg = y >= Y0 && y < Y1 && y >= u0 && y <= u1 && so != sn;
                        ent[b] = chg ? (y | (so << 24) | (sn << 28)) : -1;
                        cnt += chg ? 1 : 0;
                    }
                }
            }
            // (one reservation in the job's list per work-group and pass: an atomic per changed column -- thousands per commit
            // of the first round, all on one word -- was what the kernel waited for)
            unsigned tot;
            const unsigned incl = block_incl_add<COMMIT_NT>((unsigned)cnt, sh, tot);
            if (tid == 0 && tot) s_base = atomicAdd(&cj->nchg, (int)tot);
            __syncthreads();
            if (cnt) {
                int w_ = s_base + (int)(incl - (unsigned)cnt);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    if (ent[b] < 0) continue;
                    const int e_ = ent[b];
                    const int y = e_ & 0xffffff, so = (e_ >> 24) & 15, sn = (e_ >> 28) & 15;
                    list[w_++] = e_;
                    touch(y, 0);
                    if (so < 4 && sn >= 4 && st.tally[order[y]].w[4] == 1u) {      // the row's base was the column's last: W_Con will drop it
                        event(2 * y, -1);
                        atomicAdd(&cj->ndel, 1);
                        touch(y, -1);
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Which jobs of the batch commit (one thread; every work-group of k_commit_finish works it out for itself, from data nothing
// in the batch changes before that kernel's last work-group, when all have arrived).  Jobs in row order.  A stale job -- something a job committed
// before it changes lies in its interval -- is left for the next batch, and a later job may still commit AHEAD of it when the
// two commute: their band intervals are disjoint (with a margin for the column a commit may open at its interval's edge, and
// for the columns the commits before have opened or emptied inside the stale row's interval, which its NEXT gather will see
// shifted by as many).  The DP depends on absolute positions only through the clamps at the MSA's edges, which disjoint
// intervals rule out (commutation probe), so realigning j after i gives the state the reference reaches with j before i.
// (skipped: MAXJ words of the caller's, in LDS -- as an array of this function's it was the kernel's only scratch memory)
__device__ void commit_decide(const DState &st, const JobBufs &jb, int njobs, BatchPlan *p, const JobMeta *metas, const CommitJob *cjobs, const int *pair_cf, const int *pair_left, int *skipped)
{
    const Hdr *h = st.hdr;
    p->idle = (h->status != 0 || h->need_grow) ? 1 : 0;
    p->ncommit = p->nnew = p->ndel = p->nev = p->restructure = p->big = 0;
    p->live_all = p->live_done = p->ahead_n = 0;
    p->first = 0x7fffffff;
    p->done_mask = 0ull;
    for (int i = 0; i < 4; ++i) p->reasons[i] = 0;
    for (int j = 0; j < njobs && j < MAXJ; ++j) p->verdict[j] = V_NONE;
    if (p->idle) return;
    const int W = h->W, H = st.H, B = st.B;
    int net = 0, evabs = 0, nskip = 0;
    bool stopped = false;
    for (int j = 0; j < njobs && j < MAXJ; ++j) {
        const JobMeta *m = &metas[j];
        if (!m->active) break;                                                    // the batch ends here
        if (m->L > 0) {
            p->live_all += 1;
            if (stopped) { p->verdict[j] = V_AFTER_STOP; continue; }
            if (!m->ok) { p->verdict[j] = V_STOP_NOTOK; stopped = true; continue; }            // status already set
            // room for the columns this commit may open?  (the host regrows the arrays and the batch is repeated)
            if ((long long)W + p->nnew + m->L + 64 > st.colcap || (long long)h->nslots + p->nnew + m->L + 64 > st.slotcap) { p->verdict[j] = V_STOP_GROW; stopped = true; continue; }
            if (m->wide && !jb.f64_follows) { p->verdict[j] = V_STOP_WIDE; stopped = true; continue; }   // (its batch came without k_fill64: the next ones bring it)
            if (m->abort) { p->verdict[j] = V_STOP_ABORT; stopped = true; continue; }
            if (m->segfail) {
                // its fill is repeated with a longer warm-up in the next batch.  `fail_stops` 1 (default): the batch ends here, as up
                // to round 3.  0: until then it is a row like a stale one, and a later row that commutes with it may commit ahead
                // of it -- 0.7 % faster on the benchmark and green in every test, but NOT the default: the randomised sweep has one
                // case (scripts/dev/stress.py 25 2024 39: 64 jobs per batch, every renumbering by the pass over the width, many failed
                // checks) that ends in an inconsistent traceback with it and runs clean without; unresolved
                p->verdict[j] = V_STOP_SEGFAIL;
                if (jb.fail_stops || nskip >= MAXJ) stopped = true; else skipped[nskip++] = j;
                continue;
            }
            bool good = true;
            int why = -1;
            int d = 0, r = 0;                                                     // columns the jobs committed before open (net) left / right of this job's interval
            for (int t = 0; t < p->ncommit && good; ++t) {
                const int i = p->cjobs[t];
                const CommitJob *ci = &cjobs[i];
                if (!ci->scanned) continue;                                       // (committed without a change)
                if (pair_cf[(size_t)i * njobs + j]) { good = false; why = 3; break; }
                const int neti = metas[i].nnew - ci->ndel;
                int left;
                if (ci->u1 < m->lo - 1) left = neti;                              // all its events lie left of the interval's margin
                else if (m->hi + 1 < ci->u0 - 1) left = 0;                        // ... right of it
                else left = pair_left[(size_t)i * njobs + j];
                d += left; r += neti - left;
            }
            if (good && (d != 0 || r != 0)) {
                const int *way = jb.way + (size_t)j * jb.Lmax;
                const int way0 = way[0], wayL = way[m->L - 1];
                if (d != 0 && !(way0 - H >= 1 && way0 + d - H >= 1)) { good = false; why = 1; }           // left clamp PW:1496
                const int aL = max(0, wayL - H);
                const bool far_old = aL + B <= m->W - 1, far_new = aL + d + B <= W + net - 1;
                if (good && !(far_old && far_new) && r != 0) { good = false; why = 2; }                   // right clamp PW:1497/1505
            }
            for (int t = 0; t < nskip && good; ++t) {
                const JobMeta *ms = &metas[skipped[t]];
                if (!(m->hi + 2 + evabs < ms->lo || ms->hi + 2 + evabs < m->lo)) good = false;
            }
            // a row that was picked AHEAD of rows that are not in the batch at all (k_commit_finish of the batch before): it commutes
            // with them as long as the columns this batch has opened or emptied so far cannot have closed the gap it was picked for
            const bool jumped = st.bplan[0] && j < PLAN_MAX && st.bplan[1 + PLAN_MAX + j] != 0x7fffffff;
            if (good && jumped && st.bplan[1 + PLAN_MAX + j] <= 2 + evabs) good = false;
            if (!good) {
                if (why >= 0) p->reasons[why] += 1;
                if (nskip >= MAXJ) { p->verdict[j] = V_AFTER_STOP; stopped = true; continue; }
                skipped[nskip++] = j;
                p->verdict[j] = V_STALE;
                continue;
            }
            p->verdict[j] = V_COMMIT;
            p->cjobs[p->ncommit] = j; p->slotbase[p->ncommit] = p->nnew;
            p->ncommit += 1;
            const CommitJob *cj = &cjobs[j];
            if (cj->scanned) {
                p->nnew += m->nnew; p->ndel += cj->ndel; p->nev += cj->nev;
                net += m->nnew - cj->ndel; evabs += cj->nev;
                if (m->nnew > 0 || cj->ndel > 0) { p->restructure = 1; p->first = min(p->first, cj->first); }
                if (cj->nev > EVCAP) p->big = 1;
            }
            p->live_done += 1;
            if (nskip > 0 || jumped) p->ahead_n += 1;
        } else p->verdict[j] = V_EMPTY;                                           // (a row without bases, PW:1488, is done wherever it stands)
        if (m->off < 64) p->done_mask |= 1ull << m->off; else stopped = true;
    }
    if (p->nev > jb.evcap || p->nev > EVCAP) p->big = 1;
    if (!p->restructure) p->big = 0;
}

// the events of the committing jobs, sorted by position (key 2y: column y is emptied, 2y+1: a column opens after y); an old
// ordinal y moves by the sum of the events with key < 2y (scum: the running sums); del: the emptied ordinals, in order
__device__ void commit_sort_events(const JobBufs &jb, const BatchPlan *p, const CommitJob *cjobs, CommitEv *ev)
{
    const int tid = threadIdx.x;
    int base = 0;
    for (int t = 0; t < p->ncommit; ++t) {
        const int j = p->cjobs[t];
        const CommitJob *cj = &cjobs[j];
        if (!cj->scanned) continue;
        const int n = min(cj->nev, EVCAP);
        for (int e = tid; e < n && base + e < EVCAP; e += COMMIT_NT) { ev->key[base + e] = jb.evkey[(size_t)j * EVCAP + e]; ev->dl[base + e] = jb.evdl[(size_t)j * EVCAP + e]; }
        base += n;
    }
    const int nev = min(base, EVCAP);
    __syncthreads();
    for (int e = tid; e < nev; e += COMMIT_NT) {                                   // rank sort (nev is small)
        const int ke = ev->key[e];
        int r = 0;
        for (int f = 0; f < nev; ++f) { const int kf = ev->key[f]; r += (kf < ke || (kf == ke && f < e)) ? 1 : 0; }
        ev->skey[r] = ke; ev->scum[r] = ev->dl[e];
    }
    __syncthreads();
    if (tid == 0) {
        int cum = 0, ndel = 0;
        for (int e = 0; e < nev; ++e) {
            cum += ev->scum[e];
            ev->scum[e] = cum;
            if (!(ev->skey[e] & 1)) ev->del[ndel++] = ev->skey[e] >> 1;
        }
        ev->cum = cum; ev->nev = nev; ev->ndel = ndel;
    }
    __syncthreads();
}

// The decision, the changes, the renumbering, then -- by the work-group that arrives last, when every other one has finished --
// the header: the width, the k loop's row pointer (PW:1695 lives on the device), the size of the next batch.  A batch costs as
// long as its longest fill, and rows that overlap the rows before them are almost always invalidated while the MSA is still
// moving, so speculate just past the running mean of rows committed per batch -- and never let a speculative row make the batch
// longer than its first row, the only one that is certain to commit.
// NO work-group may leave before it has taken its ticket, whatever the batch holds: the ticket would stay one short, no header
// would be written and the host's poll would run into its bound.
__global__ __launch_bounds__(COMMIT_NT) void k_commit_finish(DState st, JobBufs jb, int njobs, const int *rowids, Hdr *host_copy, unsigned host_seq)
{
    __shared__ BatchPlan sp;
    __shared__ CommitEv ev;
    __shared__ JobMeta s_meta[MAXJ];
    __shared__ CommitJob s_cj[MAXJ];
    __shared__ int s_pcf[16 * 16], s_plf[16 * 16], s_skip[MAXJ];
    __shared__ unsigned sh[COMMIT_NT / 64];
    __shared__ int s_last, s_free, s_w;
    __shared__ int s_pl[8], s_plo[64], s_phi[64], s_pL[64], s_pgap[64];
    __shared__ unsigned long long s_ahead, s_okm, s_jm;
    __shared__ unsigned s_ev;
    __shared__ int s_bp[JR_BASE], s_sel[PLAN_MAX + 1], s_gp[PLAN_MAX + 1];
    __shared__ __attribute__((aligned(16))) int s_hw[(sizeof(Hdr) + 3) / 4];
    __shared__ int s_cw0[PLAN_CAND], s_cwL[PLAN_CAND], s_cL[PLAN_CAND], s_oldnext, s_rowend;
    const int tid = threadIdx.x;
    Hdr *h = st.hdr;
    const BatchPlan *p = &sp;
    if (tid == 0) s_pl[0] = 0;
    // the header as the batch found it (the last arriver writes it when every work-group has read it)
    const int W = h->W, cur = h->cur, agree = h->agree;
    const int nfree = h->nfree, nslots = h->nslots;
    const int *order = cur ? st.order1 : st.order0;
    int *norder = cur ? st.order0 : st.order1;
    {
        // what the decision reads, fetched by all threads at once (one thread walking it through dependent loads took as long
        // as the rest of the kernel)
        const int nj = min(njobs, MAXJ);
        for (int i = tid; i < nj * (int)(sizeof(JobMeta) / 4); i += COMMIT_NT) reinterpret_cast<int *>(s_meta)[i] = reinterpret_cast<const int *>(jb.meta)[i];
        for (int i = tid; i < nj * (int)(sizeof(CommitJob) / 4); i += COMMIT_NT) reinterpret_cast<int *>(s_cj)[i] = reinterpret_cast<const int *>(jb.cjob)[i];
        if (njobs <= 16) for (int i = tid; i < njobs * njobs; i += COMMIT_NT) { s_pcf[i] = jb.pair_cf[i]; s_plf[i] = jb.pair_left[i]; }
        __syncthreads();
        if (tid == 0) commit_decide(st, jb, njobs, &sp, s_meta, s_cj, njobs <= 16 ? s_pcf : jb.pair_cf, njobs <= 16 ? s_plf : jb.pair_left, s_skip);
    }
    __syncthreads();
    const int take = min(sp.nnew, nfree);
    const int gt = (int)blockIdx.x * COMMIT_NT + tid, GT = (int)gridDim.x * COMMIT_NT;
    const bool work = !sp.idle && sp.ncommit > 0;
    const bool fast = work && sp.restructure && !sp.big;                           // the order is renumbered from the list of events
    // (the stretch of the order this thread will copy, asked for now: the loads are under way while the changes are made and
    // the events sorted)
    constexpr int CPY = 4;
    const int s0 = max(0, min(sp.first, agree));
    int cslot[CPY];
#pragma unroll
    for (int u = 0; u < CPY; ++u) { const int y = s0 + gt + u * GT; cslot[u] = (fast && y < W) ? order[y] : 0; }
    // ---- the changes of the committing jobs, this work-group's share.  Every order[...] below reads the CURRENT buffer, which
    // nobody writes in this launch.  (What the jobs are is read from the copies in LDS: no kernel writes it after the scan.)
    for (int t = 0; work && t < sp.ncommit; ++t) {
        const int job = sp.cjobs[t];
        const JobMeta *m = &s_meta[job];
        const CommitJob *cj = &s_cj[job];
        if (!cj->scanned) continue;                                                // every base stays where it was
        const int k = m->k, L = m->L;
        const long long off = st.rowoff[k];
        const int *way = jb.way + (size_t)job * jb.Lmax;
        const int *newcol = jb.newcol + (size_t)job * jb.Lmax;
        int *aux = jb.aux + (size_t)job * jb.Lmax;
        const int *insidx = jb.insidx + (size_t)job * jb.Lmax;
        // 1. new columns (PW:1245-1332: the row's base, and AlGapCount on every entry but the gaps', PW:1320-1325) and the slot of
        //    every base (into `pos` at once: nothing else reads this row's)
        for (int x = gt; x < L; x += GT) {
            const int c = newcol[x];
            const int y = c >> 1;
            int slot = order[y];
            if (c & 1) {
                const int idx = sp.slotbase[t] + insidx[x];
                slot = (idx < take) ? st.freelist[nfree - 1 - idx] : nslots + (idx - take);
                const int bs = (int)st.seq[off + x];
                const uint32_t al = (uint32_t)aux[x];
                Tally nt;
#pragma unroll
                for (int b = 0; b < 6; ++b) nt.w[b] = ((b != bs) ? 1u : 0u) + ((b != 4) ? al : 0u);
                nt.endcnt = (x == L - 1) ? 1u : 0u; nt.pad = 0;
                st.tally[slot] = nt;
                if (sp.big) atomicAdd(&st.inscnt[y], 1);                           // (only the pass over the width reads it, and clears it)
            }
            aux[x] = slot;
            st.pos[off + x] = slot;
            if (x == L - 1) {
                const int oend = order[way[L - 1]];
                if (oend != slot) { atomicSub(&st.tally[oend].endcnt, 1u); if (!(c & 1)) atomicAdd(&st.tally[slot].endcnt, 1u); }
            }
        }
        // 2. Columns_Downdater + Column_Updater fused (PW:1172-1243) for the columns whose symbol for this row changes (the six
        //    tallies only: the ends' count of the same record is kept by atomics)
        const int nchg = cj->nchg;
        const int *list = jb.chg + (size_t)job * jb.colcap;
        for (int i = gt; i < nchg; i += GT) {
            const int e_ = list[i];
            const int y = e_ & 0xffffff, so = (e_ >> 24) & 15, sn = (e_ >> 28) & 15;
            Tally *tp = &st.tally[order[y]];
            const uint4 a = *reinterpret_cast<const uint4 *>(&tp->w[0]);
            const uint2 b2 = *reinterpret_cast<const uint2 *>(&tp->w[4]);
            uint32_t w[6] = {a.x, a.y, a.z, a.w, b2.x, b2.y};
#pragma unroll
            for (int b = 0; b < 6; ++b) w[b] = w[b] - ((so != 5 && b != so) ? 1u : 0u) + ((sn != 5 && b != sn) ? 1u : 0u);
            *reinterpret_cast<uint4 *>(&tp->w[0]) = make_uint4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<uint2 *>(&tp->w[4]) = make_uint2(w[4], w[5]);
        }
        // the row is one piece from now on: its inner segment ends are no ends any more (nbrk[k] is cleared with the header)
        const int nb = st.nbrk[k];
        const int *bx = st.brkx + st.brkoff[k];
        for (int i = gt; i < nb; i += GT) atomicSub(&st.tally[order[way[bx[i]]]].endcnt, 1u);
    }
    if (fast) {
        // ---- W_Con (PW:706-763) + splice, from the list of events: the order is written into the OTHER buffer, under the new
        // ordinals.  In place, source and target ranges overlap across work-groups (it took a launch to copy the stretches that
        // move out and another to bring them back); this way nothing that a work-group still reads is overwritten.  The other
        // buffer holds the order of two renumberings ago and equals this one only on [0, agree): everything from
        // min(first, agree) on is written, moved or not.  Every work-group sorts the events for itself.
        commit_sort_events(jb, &sp, s_cj, &ev);
        const int nev = ev.nev;
        auto place = [&](int y, int slot) {
            int a = 0, b = nev;                                                     // events with key < 2y
            while (a < b) { const int mid = (a + b) >> 1; if (ev.skey[mid] < 2 * y) a = mid + 1; else b = mid; }
            if (a < nev && ev.skey[a] == 2 * y) return;                             // emptied: its slot goes to the free list (below)
            const int shy = a ? ev.scum[a - 1] : 0;
            norder[y + shy] = slot;
            if (shy) st.rank[slot] = y + shy;
        };
#pragma unroll
        for (int u = 0; u < CPY; ++u) { const int y = s0 + gt + u * GT; if (y < W) place(y, cslot[u]); }
        for (int y = s0 + gt + CPY * GT; y < W; y += GT) place(y, order[y]);        // (more than 131 072 columns to copy)
        // the new columns: after old ordinal y, before any column opened there by a later base of the same row (PW:1245-1332);
        // aux[x] is the slot this very thread gave the base above
        for (int t = 0; t < p->ncommit; ++t) {
            const int job = p->cjobs[t];
            if (!s_cj[job].scanned || s_meta[job].nnew == 0) continue;
            const int L = s_meta[job].L;
            const int *newcol = jb.newcol + (size_t)job * jb.Lmax;
            const int *aux = jb.aux + (size_t)job * jb.Lmax;
            for (int x = gt; x < L; x += GT) {
                const int c = newcol[x];
                if (c & 1) {
                    const int y = c >> 1;
                    int tt = 0;
                    for (int xx = x - 1; xx >= 0 && newcol[xx] == c; --xx) ++tt;   // earlier bases opened there too
                    int a = 0, b = nev;                                             // events with key < 2y
                    while (a < b) { const int mid = (a + b) >> 1; if (ev.skey[mid] < 2 * y) a = mid + 1; else b = mid; }
                    const int shy = a ? ev.scum[a - 1] : 0;
                    const int kept = (a < nev && ev.skey[a] == 2 * y) ? 0 : 1;      // y itself emptied by this batch?
                    const int pnew = y + shy + kept + tt;
                    norder[pnew] = aux[x]; st.rank[aux[x]] = pnew;
                }
            }
        }
    }
    // ---- the last work-group to get here goes on
    // (every wave's stores are drained and the work-group's barrier passed before ONE lane releases them and takes a ticket;
    // the last arriver's lane acquires before anybody of its work-group reads on)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = __hip_atomic_fetch_add(jb.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
        if (s_last) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    }
    __syncthreads();
    if (!s_last) return;
    if (fast) {
        // the slots of the emptied columns (the free list's top is what the work-groups took the new columns' slots from: it
        // is written only now that all of them have), from this work-group's own sorted events
        for (int i = tid; i < ev.ndel; i += COMMIT_NT) st.freelist[nfree - take + i] = order[ev.del[i]];
        if (tid == 0) s_w = W + ev.cum;
    } else if (work && sp.restructure) {
        // the same by a pass over the width (more than evcap events; one work-group, and every work-group's tallies and
        // counts of new columns are in): new ordinal of every surviving / new column.
        // Columns left of the first one that changes keep their ordinal, and the other order buffer already holds them as far
        // as the two agree, so the renumbering starts there
        if (tid == 0) s_free = 0;
        __syncthreads();
        unsigned carry = (unsigned)s0;
        for (int base = s0; base < W; base += COMMIT_NT) {
            const int y = base + tid;
            const bool valid = y < W;
            const int slot = valid ? order[y] : 0;
            const bool keep = valid && st.tally[slot].w[4] != 0;
            const unsigned ic = valid ? (unsigned)st.inscnt[y] : 0u;
            const unsigned cnt = (keep ? 1u : 0u) + ic;
            unsigned tot;
            const unsigned incl = block_incl_add<COMMIT_NT>(cnt, sh, tot);
            const int idx = (int)(carry + incl - cnt);
            carry += tot;
            if (valid) {
                st.newidx[y] = idx;
                if (keep) { norder[idx] = slot; st.rank[slot] = idx; }
                else { const int q = atomicAdd(&s_free, 1); st.freelist[nfree - take + q] = slot; }
                if (ic) st.inscnt[y] = 0;
            }
        }
        __syncthreads();
        for (int t = 0; t < p->ncommit; ++t) {
            const int job = p->cjobs[t];
            if (!s_cj[job].scanned || s_meta[job].nnew == 0) continue;
            const int L = s_meta[job].L;
            const int *newcol = jb.newcol + (size_t)job * jb.Lmax;
            const int *aux = jb.aux + (size_t)job * jb.Lmax;
            for (int x = tid; x < L; x += COMMIT_NT) {
                const int c = newcol[x];
                if (c & 1) {
                    const int y = c >> 1;
                    int tt = 0;
                    for (int xx = x - 1; xx >= 0 && newcol[xx] == c; --xx) ++tt;
                    const int keepy = st.tally[order[y]].w[4] != 0 ? 1 : 0;
                    const int q = st.newidx[y] + keepy + tt;
                    norder[q] = aux[x];
                    st.rank[aux[x]] = q;
                }
            }
        }
        if (tid == 0) s_w = (int)carry;                                            // (the new width, for the lane that writes the header)
    }
    // ---- the header.  It is worked on in LDS: fetched by all threads at once, changed by lane 0 (a walk through a dozen cache lines of
    // global memory, one dependent round trip each, was half of this kernel), written back and sent to the host by all.
    constexpr int HW = (int)(sizeof(Hdr) / 4);
    static_assert(HW <= COMMIT_NT, "one word of the header per thread");
    if (tid < HW) s_hw[tid] = reinterpret_cast<const int *>(h)[tid];
    if (tid < JR_BASE) s_bp[tid] = st.bplan[tid];                                  // (this batch's plan, for the lane that writes the header)
    __syncthreads();
    Hdr *const hh = reinterpret_cast<Hdr *>(s_hw);
    if (tid == 0) { s_oldnext = hh->next_row; s_rowend = hh->row_end; }
    __syncthreads();
    if (tid >= 64 && tid < 64 + PLAN_CAND) {
        // While lane 0 writes the header: the rows the NEXT batch may pick from, one lane each -- the 128 rows from the row
        // pointer as it stood (it moves on by at most 64): the columns of their end bases as the state is now, final for
        // this batch, and their lengths.  (These loads are four dependent round trips; beside the header's they cost nothing.)
        const int c_ = tid - 64, kk = s_oldnext + c_;
        int w0 = 0, wL = 0, L_ = -1;
        if (kk < s_rowend) {
            const int kr = rowids[kk];
            L_ = st.rowlen[kr];
            if (L_ > 0) { const long long offr = st.rowoff[kr]; w0 = st.rank[st.pos[offr]]; wL = st.rank[st.pos[offr + L_ - 1]]; }
        }
        s_cw0[c_] = w0; s_cwL[c_] = wL; s_cL[c_] = L_;
    }
    if (tid == 0) {
        *jb.ticket = 0u;
        hh->ncommitted = 0; hh->stop = 0;
        if (!p->idle) {
            int version = hh->version, nfail = 0;
            for (int j = 0; j < njobs && j < MAXJ; ++j) {
                const int v = p->verdict[j];
                if (v == V_NONE) break;
                const JobMeta *m = &s_meta[j];
                if (v == V_STOP_GROW) hh->need_grow = 1;
                else if (v == V_STOP_ABORT) {
                    // k_fill_v3 gave this job up (time-out): it is realigned again, by k_fill_v2, as are the next batches
                    hh->stalls += 1;
                    if (jb.wpNW <= 16) hh->fallback = 65; else atomicCAS(&hh->status, 0, PWR_ERR_STALL);   // (no one-work-group form of 17 waves)
                } else if (v == V_STOP_SEGFAIL) {
                    // a segment of its fill had not forgotten its start when its own rows began (k_seg_check): the row is
                    // realigned again, with the longest warm-up, then in one piece
                    // (only the FIRST such row of a batch is tracked: it is the one the next batches begin with until it has
                    // passed, so the escalation to one piece always terminates; another one is simply repeated when its turn comes)
                    hh->seg_fails += 1;
                    if (jb.hard_rows && m->level == 0) {
                        if (m->hard & 1) { hh->hard_fills += (m->hard & 2) ? 0 : 1; hh->hard_refail += (m->hard & 2) ? 0 : 1; }
                        else hh->hard_marked += 1;
                        st.hard[m->k] = min(1 << 20, st.hard[m->k] + jb.hard_up);
                    }
                    if (!nfail++) {
                        hh->noseg_level = hh->noseg_row == m->k ? hh->noseg_level + 1 : 1; hh->noseg_row = m->k;
                        if (hh->noseg_level == 1 && hh->warm_step > 0) hh->warm_cur = min(hh->warm_hi, hh->warm_cur + hh->warm_up);
                    } else if (hh->warm_step > 0) hh->warm_cur = min(hh->warm_hi, hh->warm_cur + hh->warm_up);
                } else if (v == V_STALE) hh->stop = 1;
                else if (v == V_COMMIT) {
                    const CommitJob *cj = &s_cj[j];
                    if (cj->scanned) {
                        version += 1;
                        if (cj->nchg > 0 || m->nnew > 0) hh->rows_changed += 1;
                        if (st.nbrk[m->k]) st.nbrk[m->k] = 0;
                    }
                    hh->cells_reference += m->cells;
                    if (hh->noseg_row == m->k) { hh->noseg_row = -1; hh->noseg_level = 0; }
                    else if (m->nseg > 1 && !(m->hard & 2)) hh->warm_cur = max(hh->warm_lo, hh->warm_cur - hh->warm_step);   // (a pass the long way says nothing about the short one)
                    if (jb.hard_rows && (m->hard & 1) && m->level == 0 && m->nseg > 1) {
                        if (!(m->hard & 2)) hh->hard_fills += 1;
                        st.hard[m->k] = max(0, st.hard[m->k] - jb.hard_down);
                    }
                    if (m->wide) hh->rows_wide += 1;
                }
            }
            hh->version = version;
            for (int i = 0; i < 4; ++i) hh->fail_reason[i] += (unsigned long long)p->reasons[i];
            if (p->restructure) {
                hh->W = s_w;
                hh->nslots = nslots + (p->nnew - take);
                hh->nfree = nfree - take + p->ndel;
                // the renumbering wrote the other buffer, whichever way it went: that one is the order now, and the two agree
                // on the columns left of the first one that changed
                hh->cur = cur ^ 1; hh->agree = max(0, min(p->first, W));
            }
            // the rows of this batch that were picked ahead of rows outside it and have committed: what their intervals reach
            // beyond their bases, for the check of the rows they jumped (k_gather_a)
            unsigned long long jm = hh->jumpmask;
            if (s_bp[0]) {
                for (int j = 0; j < njobs && j < PLAN_MAX; ++j) {
                    if (p->verdict[j] != V_COMMIT || s_bp[1 + PLAN_MAX + j] == 0x7fffffff) continue;
                    const JobMeta *m = &s_meta[j];
                    if (m->off >= 64) continue;
                    const int *nc = jb.newcol + (size_t)j * jb.Lmax;
                    const int c0 = nc[0], cL = nc[m->L - 1];
                    int *rec = st.bplan + JR_BASE + 4 * ((hh->next_row + m->off) & 63);
                    rec[0] = (int)(unsigned)(hh->events_total + (unsigned long long)p->nev);
                    rec[1] = ((c0 >> 1) + (c0 & 1)) - m->lo + m->nnew + 4;
                    rec[2] = m->hi - (cL >> 1) + m->nnew + 4;
                    jm |= 1ull << m->off;
                    hh->rows_jumped += 1;
                }
            }
            hh->events_total += (unsigned long long)p->nev;
            {
                int nchg = 0;
                for (int t = 0; t < p->ncommit; ++t) nchg += s_cj[p->cjobs[t]].scanned ? 1 : 0;
                if (nchg > 0) hh->evrate = 0.9f * hh->evrate + 0.1f * ((float)p->nev / (float)nchg);
            }
            const unsigned long long dm = hh->ahead | p->done_mask;
            const int adv = ~dm ? __builtin_ctzll(~dm) : 64;
            hh->jumpmask = adv >= 64 ? 0ull : jm >> adv;
            const int done = __builtin_popcountll(p->done_mask);
            hh->ncommitted = done;
            hh->next_row += adv;
            hh->ahead = adv >= 64 ? 0ull : dm >> adv;
            hh->rows_ahead += (unsigned long long)p->ahead_n;
            if (hh->fallback > 0 && jb.v2_follows) hh->fallback -= 1;
            if (hh->need64 > 0 && jb.f64_follows) hh->need64 -= 1;
            if (p->live_all > 0) hh->batches += 1;
            hh->rows_committed += (unsigned long long)p->live_done;
            hh->rows_recomputed += (unsigned long long)(p->live_all - p->live_done);
            if (hh->status == 0 && !hh->need_grow && done > 0) {
                const float ema = 0.75f * hh->ema + 0.25f * (float)done;
                hh->ema = ema;
                const int k = hh->next_row, left = hh->row_end - k;
                int nb = (int)(ema + 2.6f);
                nb = max(1, min(nb, min(hh->window, left)));
                if (left > 0) {
                    const int l0 = st.rowlen[rowids[k]];
                    for (int j = 1; j < nb; ++j)
                        if (st.rowlen[rowids[k + j]] > l0 + (int)((long long)l0 * hh->speclen / 100) + 64) { nb = j; break; }
                }
                hh->nb = nb;
                // (what the pick of the next batch's rows below starts from)
                s_pl[0] = (jb.plan_ahead && hh->window > 1 && hh->window <= PLAN_MAX && left > 0) ? 1 : 0;
                s_pl[1] = k; s_pl[2] = hh->row_end; s_pl[3] = nb; s_pl[4] = min(hh->window, left); s_pl[5] = hh->W; s_pl[6] = hh->speclen;
                s_ahead = hh->ahead;
                // rows jump only while the MSA is calm: 64 commits' worth of opened / emptied columns must stay far below the gap
                // a jump keeps, and the jumps still pending must not have seen a quarter of it already (looked up by the lanes below)
                // (... and never while 64 commits at the present rate would fill half the gap a jump keeps: a gap set far below the default
                // would otherwise be closed by ordinary rounds and end in PWR_ERR_ORDER -- found by the randomised sweep)
                s_pl[7] = hh->evrate * 100.0f < fminf((float)jb.plan_evrate_x100, jb.plan_gate_rel ? (float)jb.plan_slack * (100.0f / 128.0f) : 3.0e38f) ? 1 : 0;
                s_jm = hh->jumpmask; s_ev = (unsigned)hh->events_total;
                if (!s_pl[0]) st.bplan[0] = 0;                                     // the next rows in order
            } else if (hh->status != 0 || hh->need_grow) {
                // No plan is made for the next batch, and the one this batch ran by must not outlive it: the jobs before the one
                // that stopped the batch have committed, next_row, ahead and jumpmask have moved on by `adv`, and the plan's offsets
                // and gaps count from the row pointer as it stood.  After the regrow the next batch takes the next rows in order.
                // (The jump records behind JR_BASE stay: they belong to rows, not to the plan.)
                st.bplan[0] = 0;
            }
        }
    }
    __syncthreads();
    if (s_pl[0]) {
        // ---- the rows of the NEXT batch.  Its first row is the next one of the k loop; the others are speculation.  Round 3 took
        // the rows that follow it in order -- which commit only if the rows before them leave their intervals alone, three times
        // in ten.  But among the next 64 rows there are rows whose band interval is DISJOINT from that of every uncommitted row
        // before them: they commute with all of those (what "commit ahead" has rested on since round 2), so their
        // realignment from the present state is exact whatever the rows before them do, and they commit in this very batch.
        // They are taken first, whatever their length; the slots that are left go to the next rows in order as before.
        const int k0n = s_pl[1], kend = s_pl[2], Wn = s_pl[5];
        if (tid < 64) {
            const int kk = k0n + tid, c_ = kk - s_oldnext;                          // (its place among the rows looked up above)
            int lo_ = 0x7fffffff, hi_ = -0x7fffffff, L_ = -1;                       // (not a candidate: committed already, or beyond the slab)
            if (kk < kend && c_ < PLAN_CAND && !((s_ahead >> tid) & 1ull)) {
                L_ = s_cL[c_];
                if (L_ > 0) { lo_ = max(0, max(0, s_cw0[c_] - st.H) - 1); hi_ = min(Wn - 1, max(0, s_cwL[c_] - st.H) + st.B - 1); }   // the interval its gather will take
            }
            s_plo[tid] = lo_; s_phi[tid] = hi_; s_pL[tid] = L_;
        }
        __syncthreads();
        if (tid < 64) {
            // distance in columns to the nearest interval of an uncommitted row before it
            int gap = 0x7fffffff;
            const int lo_ = s_plo[tid], hi_ = s_phi[tid];
            for (int i = 0; i < tid; ++i) if (s_pL[i] > 0) gap = min(gap, max(lo_ - s_phi[i], s_plo[i] - hi_));
            s_pgap[tid] = gap;
            bool spent = false;                                                    // a pending jump that has seen too many events already
            if ((s_jm >> tid) & 1ull) spent = s_ev - (unsigned)st.bplan[JR_BASE + 4 * ((k0n + tid) & 63)] > (unsigned)(jb.plan_slack / 4);
            const bool calm = s_pl[7] != 0 && __ballot(spent) == 0ull;
            const unsigned long long okm = __ballot(tid > 0 && s_pL[tid] > 0 && gap > 2 + jb.plan_slack && calm);
            if (tid == 0) s_okm = okm;
        }
        __syncthreads();
        if (tid == 0) {
            const int window = s_pl[4], nb_order = min(s_pl[3], 1 + jb.spec_inorder);
            int n = 0;
            s_sel[n] = 0; s_gp[n] = 0x7fffffff; ++n;
            unsigned long long taken = 1ull;
            const int lcap = jb.plan_len > 0 ? max(0, s_pL[0]) + (int)((long long)max(0, s_pL[0]) * jb.plan_len / 100) + 64 : 0x7fffffff;
            for (unsigned long long q = s_okm & ~1ull; q && n < window; q &= q - 1) {
                const int off = __builtin_ctzll(q);
                if (s_pL[off] > lcap) continue;                                    // (test hook: a row picked ahead no longer than this)
                s_sel[n] = off; s_gp[n] = s_pgap[off]; ++n; taken |= 1ull << off;
            }
            const int l0 = max(0, s_pL[0]);
            int inorder = 1;
            for (int off = 1; off < 64 && n < window && inorder < nb_order; ++off) {
                if (s_pL[off] < 0) { if (k0n + off >= kend) break; continue; }     // committed ahead already
                if ((taken >> off) & 1ull) continue;                               // in the batch already: the run of rows goes on behind it
                if (s_pL[off] > l0 + (int)((long long)l0 * s_pl[6] / 100) + 64) break;   // never a row in order that makes the batch longer than its first
                s_sel[n] = off; s_gp[n] = 0x7fffffff; ++n; ++inorder;
            }
            for (int a = 1; a < n; ++a) {                                          // jobs in row order
                const int so = s_sel[a], sg = s_gp[a];
                int b = a - 1;
                while (b >= 0 && s_sel[b] > so) { s_sel[b + 1] = s_sel[b]; s_gp[b + 1] = s_gp[b]; --b; }
                s_sel[b + 1] = so; s_gp[b + 1] = sg;
            }
            for (int j = 0; j < n; ++j) { st.bplan[1 + j] = s_sel[j]; st.bplan[1 + PLAN_MAX + j] = s_gp[j]; }
            st.bplan[0] = 1;
            hh->nb = n;
        }
    }
    __syncthreads();
    // back to global memory, and the copy for the host: every word but the sequence number, a system-scope fence by the waves that
    // wrote, then the number -- the host polls that word, no copy command and no event record (6 us each on the stream) per batch
    if (tid < HW) reinterpret_cast<int *>(h)[tid] = s_hw[tid];
    if (host_copy) {
        constexpr int SEQW = (int)(offsetof(Hdr, seq) / 4);
        if (tid < HW && tid != SEQW) { reinterpret_cast<volatile int *>(host_copy)[tid] = s_hw[tid]; __threadfence_system(); }
        __syncthreads();
        if (tid == 0) { *reinterpret_cast<volatile unsigned *>(&host_copy->seq) = host_seq; __threadfence_system(); }
    }
}

// ---------------------------------------------------------------------------------------------
// One round split over several GPUs (pwr_split_*): what a rank's fills and tracebacks produced travels as one fixed-size
// record per job -- the job's JobMeta, its new placement newcol[Lmax], the chunk words of the traceback gtr[trk] (the commit
// reads the 'up' moves of every 64 rows from them) --, is all-gathered by the caller, and is put into the job slots of the
// ranks that did not compute it.  Everything else the commit reads (Way, the old marks, the interval, the version the inputs
// were gathered at) every rank has made itself, from its own replica of the state, with the same gather.
// ---------------------------------------------------------------------------------------------
__host__ __device__ static inline size_t split_slot_bytes(int Lmax, int trk)
{
    return (sizeof(JobMeta) + (size_t)Lmax * 4 + (size_t)trk * 8 + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(256) void k_split_export(JobBufs jb, int njobs, unsigned char *out)
{
    const int job = blockIdx.x, tid = threadIdx.x;
    if (job >= njobs || NOT_MINE(jb, job)) return;
    unsigned char *slot = out + (size_t)(job / jb.split_world) * split_slot_bytes(jb.Lmax, jb.trk);
    const JobMeta *m = &jb.meta[job];
    if (tid < (int)(sizeof(JobMeta) / 4)) reinterpret_cast<int *>(slot)[tid] = reinterpret_cast<const int *>(m)[tid];
    if (!m->active || m->L <= 0) return;
    int *nc = reinterpret_cast<int *>(slot + sizeof(JobMeta));
    const int *src = jb.newcol + (size_t)job * jb.Lmax;
    for (int x = tid; x < m->L; x += 256) nc[x] = src[x];
    unsigned long long *gt = reinterpret_cast<unsigned long long *>(slot + sizeof(JobMeta) + (size_t)jb.Lmax * 4);
    const unsigned long long *gs = jb.gtr + (size_t)job * jb.trk;
    const int nch = min(jb.trk, (m->L + TB_C - 1) / TB_C);
    for (int i = tid; i < nch; i += 256) gt[i] = gs[i];
}

__global__ __launch_bounds__(256) void k_split_import(DState st, JobBufs jb, int njobs, const unsigned char *in)
{
    const int job = blockIdx.x, tid = threadIdx.x;
    if (job >= njobs || !NOT_MINE(jb, job)) return;
    const int slots_per_rank = (njobs + jb.split_world - 1) / jb.split_world;
    const unsigned char *slot = in + ((size_t)(job % jb.split_world) * slots_per_rank + (size_t)(job / jb.split_world)) * split_slot_bytes(jb.Lmax, jb.trk);
    const JobMeta *src = reinterpret_cast<const JobMeta *>(slot);
    JobMeta *m = &jb.meta[job];
    // the replicas must agree on what the job is: same row, same length, gathered from the same version of the state
    if (src->active != m->active || (m->active && (src->k != m->k || src->L != m->L || src->ver != m->ver || src->lo != m->lo || src->hi != m->hi))) {
        if (tid == 0) atomicCAS(&st.hdr->status, 0, PWR_ERR_INTERNAL);
        return;
    }
    if (!m->active || m->L <= 0) return;
    const int L = m->L;
    __syncthreads();
    if (tid == 0) {
        // what the owner's fill and traceback wrote (everything else is this rank's own gather)
        m->entry = src->entry; m->ok = src->ok; m->nnew = src->nnew; m->abort = src->abort; m->changed = src->changed;
        m->segfail = src->segfail; m->nseg = src->nseg; m->clk = src->clk; m->rclk = src->rclk; m->rounds = src->rounds;
        if (!src->ok) atomicCAS(&st.hdr->status, 0, PWR_ERR_INTERNAL);               // (the owner's traceback found "Stuff gone wrong")
    }
    const int *nc = reinterpret_cast<const int *>(slot + sizeof(JobMeta));
    int *dst = jb.newcol + (size_t)job * jb.Lmax;
    for (int x = tid; x < L; x += 256) dst[x] = nc[x];
    const unsigned long long *gt = reinterpret_cast<const unsigned long long *>(slot + sizeof(JobMeta) + (size_t)jb.Lmax * 4);
    unsigned long long *gd = jb.gtr + (size_t)job * jb.trk;
    const int nch = min(jb.trk, (L + TB_C - 1) / TB_C);
    for (int i = tid; i < nch; i += 256) gd[i] = gt[i];
}

// ---------------------------------------------------------------------------------------------
// total score (PW:864-892, PW:933-963): sum over columns of sum_b n_b * (cov - n_b), n_b = cov - w[b]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_score(DState st, unsigned long long *out)
{
    __shared__ unsigned long long sh[4];
    const int W = st.hdr->W;
    const int *order = cur_order(st);
    unsigned long long s = 0;
    for (int y = blockIdx.x * blockDim.x + threadIdx.x; y < W; y += gridDim.x * blockDim.x) {
        const Tally t = st.tally[order[y]];
#pragma unroll
        for (int b = 0; b < 5; ++b) s += (unsigned long long)(t.w[5] - t.w[b]) * (unsigned long long)t.w[b];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, sh[0] + sh[1] + sh[2] + sh[3]);
}

// MMA_Auslesen (PW:1556-1598): one work-group per row writes "ACGT- " text
__global__ __launch_bounds__(256) void k_export(DState st, unsigned char *out, int row0, int nrows, int W, int nl)
{
    const int r = row0 + blockIdx.x;
    if (blockIdx.x >= nrows) return;
    unsigned char *o = out + (size_t)blockIdx.x * (size_t)(W + nl);                    // nl 1: the row's line of the FILE (PW:1594)
    if (nl && threadIdx.x == 0) o[W] = '\n';
    const int L = st.rowlen[r];
    const long long off = st.rowoff[r];
    for (int y = threadIdx.x; y < W; y += blockDim.x) o[y] = ' ';
    __syncthreads();
    if (L == 0) return;
    const int s = st.rank[st.pos[off]], e = st.rank[st.pos[off + L - 1]];
    for (int y = s + threadIdx.x; y <= e; y += blockDim.x) o[y] = '-';
    __syncthreads();
    for (int x = threadIdx.x; x < L; x += blockDim.x) o[st.rank[st.pos[off + x]]] = "ACGT"[st.seq[off + x]];
    const int nb = st.nbrk[r];
    if (nb) {
        __syncthreads();
        const int *bx = st.brkx + st.brkoff[r];
        for (int t = threadIdx.x; t < nb; t += blockDim.x)
            for (int y = st.rank[st.pos[off + bx[t]]] + 1; y < st.rank[st.pos[off + bx[t] + 1]]; ++y) o[y] = ' ';
    }
}

// introspection (tests): ordinals of the bases of one row
__global__ __launch_bounds__(256) void k_rowcols(DState st, int k, int *out)
{
    const long long off = st.rowoff[k];
    const int L = st.rowlen[k];
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < L; x += gridDim.x * blockDim.x) out[x] = st.rank[st.pos[off + x]];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#include <climits>
#include <memory>

#define PWR_STAGE "pwr"
#include "dev_util.h"

struct pwr_ctx {
    int T = 0, B = 0, H = 0, device = 0;
    // host-side text (valid while !on_device)
    int W_host = 0;
    std::vector<unsigned char> text;      // symbol codes 0..5, row-major T x W_host
    bool on_device = false;
    // device
    DState st{};
    JobBufs jb{};
    int njobs = 0;
    int *d_jobrows = nullptr;
    int *d_rowids = nullptr;              // the rows of the k loop in order -- the rows that HAVE bases (a row without any is done wherever it stands, PW:1488; the sections
                                          // of a Window.py cut are half made of them): job j of a batch that begins at position p realigns d_rowids[p + off_j]
    std::vector<int> ids, pos_lo;         // ... on the host; pos_lo[r] = how many rows before row r have bases (T + 1 entries)
    unsigned long long *d_score = nullptr;
    hipStream_t stream = nullptr;
    std::vector<int> rowlen;
    long long sumL = 0;
    int Lmax = 0;
    // options
    int window = 3;
    double batch_ema = 1.0;               // running mean of rows committed per batch (sizes the next one)
    int profile = 0;
    unsigned gather_tag = 0;              // launch counter of the gather
    int force64 = 0;                      // test hook: every job takes k_fill64
    int evcap = EVCAP;                    // test hook: event-list renumbering up to this many structural events per commit
    int stall_test = 0;                   // test hook: this many k_fill_v3 launches have their first job stall
    int par_trace = 2;                    // 2: one wave per 64 rows, hand-over without a chain (k_trace_blk); 1: 64 chunks handing over top-down (k_trace_par); 0: single-wave k_trace_wp
    int cap_slack = 8192;                 // 0 = allocate tightly (tests: forces the regrow path)
    int spec_len = 6;                     // percent a speculative row may be longer than the first row of its batch (option "spec_len")
    int fill_mode = 4;                    // 4: k_fill_v3 (one work-group per wave, default), 3: k_fill_v2 (one work-group per DP; cross-check and fallback)
    double host_enqueue_s = 0, host_wait_s = 0;   // diagnostic: time the host spent enqueueing batches / waiting for their headers (read-only options)
    long grows = 0, grows_mid_batch = 0;          // regrows of the column arrays; those of them after earlier jobs of the same batch had committed (read-only options)
    unsigned host_seq = 0;                // sequence number of the header copies the commit kernels leave in pinned memory
    int seen_fallback = 0, seen_need64 = 0;   // Hdr::fallback / need64 as the host last saw them: the batches it enqueues bring k_fill_v2 / k_fill64 along
    int trace_epoch = 0;                  // k_trace_par launch counter (22 bits)
    int fill_epoch = 0;                   // k_fill_v3 launch counter (15 bits; the mailboxes are cleared when it wraps)
    int wave_cols = 0;                    // 4 with 9 waves: 256-column strips also at bandwidths up to 1000, so that no wave has two strips of a DP row (experiment)
    int wp_waves = 5;                     // waves per DP of the wave-pipeline fills: 9/8/5/4/3 with 2/3/4/6/8 columns per lane (5: measured best with segments side by side)
    int one_wg = 0;                       // k_fill_v3: the waves of a segment as one work-group (hand-over through LDS); 0: one work-group per wave
    int one_wg_lds = 0;                   // ... with this many bytes of dynamic LDS on top (keeps other work-groups off its compute unit)
    int fill_lds = 0;                     // experiment: dynamic LDS per work-group of the default fill (bounds the work-groups per compute unit)
    int seg_rows = 160;                   // k_fill_v3: a DP is filled in segments of about this many rows, side by side (0: in one piece)
    int seg_align = 16;                   // ... whose own parts start at multiples of this many rows (16 / 32 / 64)
    int seg_max = 64;                     // ... at most this many per DP (<= SEG_MAX)
    int seg_budget = 0;                   // > 0: this many for all the jobs of a batch together, dealt by length (measured slower; 0: seg_rows rows each)
    int seg_minrows = 64;                 // ... none with fewer own rows than this
    int spec_inorder = 64, plan_gate_rel = 1, plan_len = 0;
    int trace_prior = 1;                  // k_trace_blk: a run of rows whose record says 'stay where you are' is one step of a pass, not one per row (0: every row is stepped, as up to round 6)
    int check_in_trace = 1;               // the work-groups of k_seg_check ride in k_trace_blk's launch (0: a launch of their own, as up to round 4's first half)
    int fail_stops = 1, hard_rows = 1, hard_up_pm = 300, hard_down_pm = 0;   // (per mille of the bandwidth)
    int plan_slack = PLAN_SLACK, plan_evrate_x100 = (int)(PLAN_EVRATE_MAX * 100.0f);   // test hooks: the gap a row must keep to be picked ahead, the event rate above which none is
    int plan_ahead = 1;                   // the speculative rows of a batch: rows among the next 64 whose interval is disjoint from every uncommitted row before them first (0: the next rows in order)
    int seg_balance = 0;                  // 1: ... cut so that every segment runs about as many rows as the others, its warm-up included (measured slower)
    int split_rank = 0, split_world = 1;  // pwr_split_*: this context is replica split_rank of split_world (one per GPU)
    int split_k0 = 0, split_kend = 0;     // ... rows of the slab in progress
    int src_start = 1;                    // ... from the column of the base before the warm-up's first row alone (0: from the free start)
    int warm_pct = 190;                   // ... each warmed up while the band moves by this many percent of the bandwidth -- at most: with
    int warm_adapt = 1;                   // "warm_adapt" (and src_start) the length is steered between warm_min_pct and warm_pct by the
    int warm_min_pct = 100;               // failures of the check (Hdr::warm_cur)
    int warm_down_pm = 5, warm_up_pm = 50;  // ... per mille of the bandwidth a fill that passes takes off / one that fails puts back on
    // stats
    pwr_stats stats{};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    void *h_hdr = nullptr;                // pinned staging buffer for the device header
    void *h_ring = nullptr;               // pinned copies of the header, one per batch in flight
    // pwr_snapshot_*: the file image of the state, copied out on a stream of its own (buffers kept between snapshots)
    unsigned char *snap_dev = nullptr, *snap_host = nullptr;
    size_t snap_cap = 0;
    hipStream_t snap_stream = nullptr;
    hipEvent_t snap_taken = nullptr, snap_done = nullptr;
    bool snap_busy = false;
    // all device allocations, for cleanup
    std::vector<void *> allocs;
    std::vector<void *> job_allocs;       // ... those of them that alloc_jobs made and free_jobs frees
};
struct pwr_snapshot { pwr_ctx *c; int rows, width; size_t bytes; };

// Every option of pwr_set_option / pwr_get_option that is a field of the context, once: its key, the field, the values it
// takes (lo .. hi; with nof > 0 only the nof values of `of`), whether it is refused once the state is on the device, and
// the copy of it in JobBufs where the kernels read it (set with the field, and by alloc_jobs after every regrow).
struct Option {
    const char *key;
    int pwr_ctx::*field;
    long lo, hi;
    bool host_only;
    int JobBufs::*mirror;
    int nof;
    int of[6];
};
static const Option OPTIONS[] = {
    // (capped: every work-group of a k_fill_v3 launch must be resident at once -- 9 of 128 threads per job -- and a
    // window beyond what one CU-full of jobs survives is of no use anyway)
    {"window", &pwr_ctx::window, 1, 128, true},
    {"profile", &pwr_ctx::profile, 0, 1000000},
    {"spec_len", &pwr_ctx::spec_len, 0, 100000},
    {"fill", &pwr_ctx::fill_mode, 3, 4, true},
    {"stall_test", &pwr_ctx::stall_test, 0, 1000000},
    {"evcap", &pwr_ctx::evcap, 0, EVCAP, false, &JobBufs::evcap},
    {"force64", &pwr_ctx::force64, 0, 1, false, &JobBufs::force64},
    {"ptrace", &pwr_ctx::par_trace, 0, 2},
    {"slack", &pwr_ctx::cap_slack, 0, INT_MAX, true},
    // (test hooks: where the launch counters behind the mailbox / hand-over tags stand, so that their wrap-around can be exercised)
    {"fill_epoch", &pwr_ctx::fill_epoch, 0, (1 << 15) - 1},
    {"trace_epoch", &pwr_ctx::trace_epoch, 0, (1 << 14) - 1},
    {"onewg", &pwr_ctx::one_wg, 0, 1},
    {"fill_lds", &pwr_ctx::fill_lds, 0, 100000},
    {"onewg_lds", &pwr_ctx::one_wg_lds, 0, 100000},
    {"seg_rows", &pwr_ctx::seg_rows, 0, 1000000, true},
    {"seg_align", &pwr_ctx::seg_align, 16, 64, true, &JobBufs::seg_align, 3, {16, 32, 64}},
    {"seg_max", &pwr_ctx::seg_max, 1, SEG_MAX, true},
    {"seg_budget", &pwr_ctx::seg_budget, 0, 100000, false, &JobBufs::seg_budget},
    {"plan_slack", &pwr_ctx::plan_slack, 0, 1000000, false, &JobBufs::plan_slack},
    {"hard_rows", &pwr_ctx::hard_rows, 0, 2, true, &JobBufs::hard_rows},
    {"hard_up_pm", &pwr_ctx::hard_up_pm, 1, 100000, true},
    {"hard_down_pm", &pwr_ctx::hard_down_pm, 0, 100000, true},
    {"check_in_trace", &pwr_ctx::check_in_trace, 0, 1},
    {"trace_prior", &pwr_ctx::trace_prior, 0, 1},
    {"plan_len", &pwr_ctx::plan_len, 0, 100000, false, &JobBufs::plan_len},
    {"plan_gate_rel", &pwr_ctx::plan_gate_rel, 0, 1, false, &JobBufs::plan_gate_rel},
    {"spec_inorder", &pwr_ctx::spec_inorder, 0, 64, false, &JobBufs::spec_inorder},
    {"fail_stops", &pwr_ctx::fail_stops, 0, 1, false, &JobBufs::fail_stops},
    {"plan_evrate_x100", &pwr_ctx::plan_evrate_x100, 0, 100000000, false, &JobBufs::plan_evrate_x100},
    {"plan_ahead", &pwr_ctx::plan_ahead, 0, 1, false, &JobBufs::plan_ahead},
    {"seg_balance", &pwr_ctx::seg_balance, 0, 1, false, &JobBufs::seg_balance},
    {"seg_minrows", &pwr_ctx::seg_minrows, 16, 100000, false, &JobBufs::seg_minrows},
    {"src_start", &pwr_ctx::src_start, 0, 1, true, &JobBufs::src_start},
    {"warm_adapt", &pwr_ctx::warm_adapt, 0, 1, true},
    {"warm_down_pm", &pwr_ctx::warm_down_pm, 1, 1000, true},
    {"warm_up_pm", &pwr_ctx::warm_up_pm, 1, 10000, true},
    {"warm_min_pct", &pwr_ctx::warm_min_pct, 0, 100000, true},
    {"warm_pct", &pwr_ctx::warm_pct, 0, 100000, true},
    {"wave_cols", &pwr_ctx::wave_cols, 0, 4, true, nullptr, 2, {0, 4}},
    {"waves", &pwr_ctx::wp_waves, 3, 17, true, nullptr, 6, {3, 4, 5, 8, 9, 17}},
};
static const Option *find_option(const char *key)
{
    for (const Option &o : OPTIONS)
        if (!strcmp(key, o.key)) return &o;
    return nullptr;
}

// The host's passes over the text (1.8 GB at benchmark scale: parse, EntAlGapper, the first tallies) are row-parallel:
// f(r0, r1, t) for contiguous shares of the rows on up to 16 threads.
template <class F>
static void par_rows(int T, F f)
{
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    nt = (unsigned)std::max(1, std::min<int>((int)nt, T / 64));
    if (nt <= 1) { f(0, T, 0); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([=]() { f((int)((long long)T * t / nt), (int)((long long)T * (t + 1) / nt), (int)t); });
    for (auto &x : th) x.join();
}
static unsigned par_threads(int T)
{
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    return (unsigned)std::max(1, std::min<int>((int)nt, T / 64));
}

static int code_of_char(unsigned char c)
{
    switch (c) {   // PW:165-222
    case 'a': case 'A': return 0;
    case 'c': case 'C': return 1;
    case 'g': case 'G': return 2;
    case 't': case 'T': return 3;
    case '-': case '_': return 4;
    case ' ': return 5;
    default: return -1;
    }
}

extern "C" const char *pwr_strerror(int code)
{
    switch (code) {
    case PWR_OK: return "ok";
    case PWR_ERR_ARG: return "bad argument";
    case PWR_ERR_NOMEM: return "out of memory";
    case PWR_ERR_DEVICE: return "HIP device error";
    case PWR_ERR_INPUT: return "malformed MSA input";
    case PWR_ERR_RANGE: return "limit exceeded (sequence length or bandwidth)";
    case PWR_ERR_INTERNAL: return "inconsistent traceback";
    case PWR_ERR_UNSUPPORTED: return "MSA state is not trimmed ('-' next to a blank or at an edge): pwr_trim_ends first";
    case PWR_ERR_IO: return "cannot open output file";
    case PWR_ERR_ORDER: return "a row realigned ahead of rows outside its batch no longer commutes with one of them (columns opened or emptied in between closed the gap): rerun with option plan_ahead 0";
    case PWR_ERR_STALL: return "a fill kernel wave waited too long for its neighbour work-group and this geometry has no one-work-group form";
    default: return "unknown error";
    }
}

extern "C" int pwr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return PWR_ERR_DEVICE;
    return n;
}

// (the entries of the C ABI that can allocate on the host run through abi_guard: they are at the end of the file)
static int create(pwr_ctx **out, int rows, int width, const unsigned char *text, int bandwidth, int device)
{
    if (!out || !text || rows <= 0 || width <= 0) return PWR_ERR_ARG;
    if (bandwidth < 1 || bandwidth > PWR_MAX_BANDWIDTH) return PWR_ERR_RANGE;
    std::unique_ptr<pwr_ctx> c(new pwr_ctx());
    c->T = rows; c->B = bandwidth; c->H = bandwidth / 2; c->device = device;   // PW:1625-1626
    c->W_host = width;
    c->text.resize((size_t)rows * width);
    std::vector<int> bad(par_threads(rows), 0);
    par_rows(rows, [&](int r0, int r1, int t) {
        for (size_t i = (size_t)r0 * width; i < (size_t)r1 * width; ++i) {
            const int s = code_of_char(text[i]);
            if (s < 0) { bad[t] = 1; return; }
            c->text[i] = (unsigned char)s;
        }
    });
    for (int b : bad) if (b) return PWR_ERR_INPUT;
    *out = c.release();
    return PWR_OK;
}

static void free_device(pwr_ctx *c)
{
    for (void *p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    c->job_allocs.clear();
    for (auto &e : c->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    c->ev_pool.clear();
    c->ev_used = 0;
    if (c->stream) { (void)hipStreamDestroy(c->stream); c->stream = nullptr; }
    if (c->h_hdr) { (void)hipHostFree(c->h_hdr); c->h_hdr = nullptr; }
    if (c->h_ring) {
        (void)hipHostFree(c->h_ring); c->h_ring = nullptr;
    }
    if (c->snap_stream) { (void)hipStreamSynchronize(c->snap_stream); (void)hipStreamDestroy(c->snap_stream); c->snap_stream = nullptr; }
    if (c->snap_taken) { (void)hipEventDestroy(c->snap_taken); c->snap_taken = nullptr; }
    if (c->snap_done) { (void)hipEventDestroy(c->snap_done); c->snap_done = nullptr; }
    if (c->snap_host) { (void)hipHostFree(c->snap_host); c->snap_host = nullptr; }
    c->snap_dev = nullptr; c->snap_cap = 0; c->snap_busy = false;                   // (snap_dev is in allocs)
    c->on_device = false;
}

extern "C" void pwr_destroy(pwr_ctx *c)
{
    if (!c) return;
    if (c->on_device || !c->allocs.empty()) { (void)hipSetDevice(c->device); free_device(c); }
    delete c;
}

template <typename T>
static int dmalloc(pwr_ctx *c, T **p, size_t n)
{
    void *q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return PWR_ERR_NOMEM;
    c->allocs.push_back(q);
    *p = reinterpret_cast<T *>(q);
    return PWR_OK;
}
static void dfree(pwr_ctx *c, void *p)
{
    if (!p) return;
    for (size_t i = 0; i < c->allocs.size(); ++i)
        if (c->allocs[i] == p) { c->allocs.erase(c->allocs.begin() + i); break; }
    (void)hipFree(p);
}

// Host EntAlGapper (PW:459-645) on the code matrix.  A '-' turns blank when the row is blank in the
// previous surviving column (or there is none); surviving = the column holds a base in some row.
// The test only ever looks at the same row, so each row is swept on its own, left-to-right and then
// right-to-left, over the surviving columns.
static void host_trim(pwr_ctx *c)
{
    const int T = c->T, W = c->W_host;
    const unsigned nth = par_threads(T);
    std::vector<std::vector<unsigned char>> hasp(nth, std::vector<unsigned char>(W, 0));
    par_rows(T, [&](int r0, int r1, int t) {
        unsigned char *has = hasp[t].data();
        for (int r = r0; r < r1; ++r) {
            const unsigned char *row = &c->text[(size_t)r * W];
            for (int i = 0; i < W; ++i) has[i] |= (row[i] < 4);
        }
    });
    std::vector<int> keep;
    keep.reserve(W);
    for (int i = 0; i < W; ++i) {
        unsigned char h = 0;
        for (unsigned t = 0; t < nth; ++t) h |= hasp[t][i];
        if (h) keep.push_back(i);
    }
    const int n = (int)keep.size();
    std::vector<unsigned char> nt((size_t)T * n);
    par_rows(T, [&](int r0, int r1, int) {
        for (int r = r0; r < r1; ++r) {
            const unsigned char *row = &c->text[(size_t)r * W];
            unsigned char *o = &nt[(size_t)r * n];
            bool prev_blank = true;
            for (int i = 0; i < n; ++i) {
                unsigned char s = row[keep[i]];
                if (s == 4 && prev_blank) s = 5;
                prev_blank = (s == 5);
                o[i] = s;
            }
            bool next_blank = true;
            for (int i = n - 1; i >= 0; --i) {
                if (o[i] == 4 && next_blank) o[i] = 5;
                next_blank = (o[i] == 5);
            }
        }
    });
    c->text.swap(nt);
    c->W_host = n;
}

// The geometry of the wave-pipeline fills: NW waves per segment (or per DP), each lane of a wave C columns of a strip of
// 64 * C.  settle_geometry makes the options that choose it consistent ("waves" reads back what it leaves).  with_geometry
// is the one place that turns them into the pair -- the seven pairs there are kernels for -- and calls f(NW, C) with it as
// compile-time constants: the launches (launch_fill) instantiate their kernels from it, alloc_jobs sizes the buffers.
static void settle_geometry(pwr_ctx *c)
{
    if (c->B > 1000) c->wp_waves = 9;
    if (c->wp_waves == 17 && c->fill_mode != 4) c->wp_waves = 9;          // 17 x 64 threads do not fit one work-group
    if (c->wp_waves != 9) c->wave_cols = 0;
}
template <int N> using Int = std::integral_constant<int, N>;
template <class F>
static void with_geometry(const pwr_ctx *c, F f)
{
    switch (c->wp_waves) {
    case 17: return f(Int<17>{}, Int<1>{});
    case 5: return f(Int<5>{}, Int<4>{});
    case 8: return f(Int<8>{}, Int<3>{});
    case 4: return f(Int<4>{}, Int<6>{});
    case 3: return f(Int<3>{}, Int<8>{});
    default: return (c->B <= 1024 && c->wave_cols != 4) ? f(Int<9>{}, Int<2>{}) : f(Int<9>{}, Int<4>{});
    }
}

static int alloc_jobs(pwr_ctx *c, int njobs)
{
    JobBufs &jb = c->jb;
    settle_geometry(c);
    int NW = 0, C = 0;
    with_geometry(c, [&](auto nw, auto cols) { NW = nw; C = cols; });
    const int NC = NW * 64 * C;
    const size_t first = c->allocs.size();                                 // (what is allocated from here on is what free_jobs gives back)
    jb.Lmax = std::max(c->Lmax, 1);
    for (const Option &o : OPTIONS)
        if (o.mirror) jb.*o.mirror = c->*o.field;
    jb.colcap = c->st.colcap;
    jb.NC = NC;
    jb.dirstride = (size_t)((jb.Lmax + 15) / 16) * NC;
    int rc;
    if ((rc = dmalloc(c, &jb.meta, njobs))) return rc;
    if ((rc = dmalloc(c, &jb.way, (size_t)njobs * jb.Lmax))) return rc;
    if ((rc = dmalloc(c, &jb.g64, (size_t)njobs * jb.colcap))) return rc;
    if ((rc = dmalloc(c, &jb.gpart, (size_t)njobs * GATHER_G))) return rc;
    if (hipMemsetAsync(jb.gpart, 0, sizeof(GatherPart) * (size_t)njobs * GATHER_G, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    if ((rc = dmalloc(c, &jb.rec2, (size_t)njobs * jb.colcap * 2))) return rc;
    if ((rc = dmalloc(c, &jb.mark, (size_t)njobs * jb.colcap))) return rc;
    if ((rc = dmalloc(c, &jb.mark2, (size_t)njobs * jb.colcap))) return rc;
    if ((rc = dmalloc(c, &jb.dirs, (size_t)njobs * jb.dirstride))) return rc;
    if ((rc = dmalloc(c, &jb.newcol, (size_t)njobs * jb.Lmax))) return rc;
    if ((rc = dmalloc(c, &jb.aux, (size_t)njobs * jb.Lmax))) return rc;
    if ((rc = dmalloc(c, &jb.desc, (size_t)njobs * jb.Lmax))) return rc;
    jb.wpNW = NW;
    jb.wpMS = 64 * C;
    if ((rc = dmalloc(c, &jb.lastM, (size_t)njobs * jb.NC))) return rc;
    // (derived from several options, or from an option and the fill mode)
    jb.smax = std::max(1, std::min(c->seg_max, SEG_MAX));
    jb.hard_up = std::max(1, (int)((long long)c->B * c->hard_up_pm / 1000)); jb.hard_down = (int)((long long)c->B * c->hard_down_pm / 1000);
    jb.rowids = c->d_rowids;
    jb.seg_rows = c->fill_mode == 4 ? c->seg_rows : 0;
    jb.split_rank = c->split_rank; jb.split_world = c->split_world;
    jb.warm_cols = (int)std::min<long long>((long long)c->B * c->warm_pct / 100 + 2, 1 << 20);
    jb.gstride = jb.Lmax + jb.smax * (2 * jb.warm_cols + 64);          // (a row whose check failed warms up twice as long)
    if ((rc = dmalloc(c, &jb.seg, (size_t)njobs * SEG_MAX))) return rc;
    if (hipMemsetAsync(jb.seg, 0, sizeof(SegDesc) * (size_t)njobs * SEG_MAX, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    if ((rc = dmalloc(c, &jb.chk, (size_t)njobs * (SEG_MAX + 1) * 2 * NC))) return rc;
    if (hipMemsetAsync(jb.chk, 0xff, sizeof(unsigned) * (size_t)njobs * (SEG_MAX + 1) * 2 * NC, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    if (c->fill_mode == 4) {
        const size_t nmb = (size_t)njobs * NW * jb.gstride;
        if ((rc = dmalloc(c, &jb.gmb, nmb))) return rc;
        // on the stream the kernels run on (a plain hipMemset is not ordered against it) and waited for
        if (hipMemsetAsync(jb.gmb, 0, nmb * 8, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return PWR_ERR_DEVICE;
        c->fill_epoch = 0;
    }
    jb.trk = std::max(TRK, jb.Lmax / TB_C + 1);
    if ((rc = dmalloc(c, &jb.gtr, (size_t)njobs * jb.trk))) return rc;
    if ((rc = dmalloc(c, &jb.diag, (size_t)njobs * 32 * 4096))) return rc;
    if (hipMemsetAsync(jb.diag, 0, (size_t)njobs * 32 * 4096 * 8, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    if (hipMemsetAsync(jb.gtr, 0, (size_t)njobs * jb.trk * 8, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    c->trace_epoch = 0;
    if ((rc = dmalloc(c, &c->d_jobrows, njobs))) return rc;
    if ((rc = dmalloc(c, &jb.cjob, njobs))) return rc;
    if ((rc = dmalloc(c, &jb.chg, (size_t)njobs * jb.colcap))) return rc;
    if ((rc = dmalloc(c, &jb.evkey, (size_t)njobs * EVCAP))) return rc;
    if ((rc = dmalloc(c, &jb.evdl, (size_t)njobs * EVCAP))) return rc;
    if ((rc = dmalloc(c, &jb.insidx, (size_t)njobs * jb.Lmax))) return rc;
    if ((rc = dmalloc(c, &jb.pair_cf, (size_t)njobs * njobs))) return rc;
    if ((rc = dmalloc(c, &jb.pair_left, (size_t)njobs * njobs))) return rc;
    if ((rc = dmalloc(c, &jb.ticket, 4))) return rc;
    if ((rc = dmalloc(c, &jb.chkdone, (size_t)njobs))) return rc;
    if (hipMemsetAsync(jb.chkdone, 0, sizeof(int) * (size_t)njobs, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    if (hipMemsetAsync(jb.cjob, 0, sizeof(CommitJob) * njobs, c->stream) != hipSuccess || hipMemsetAsync(jb.pair_cf, 0, sizeof(int) * (size_t)njobs * njobs, c->stream) != hipSuccess ||
        hipMemsetAsync(jb.pair_left, 0, sizeof(int) * (size_t)njobs * njobs, c->stream) != hipSuccess ||
        hipMemsetAsync(jb.ticket, 0, 16, c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    if (hipMemset(jb.meta, 0, sizeof(JobMeta) * njobs) != hipSuccess) return PWR_ERR_DEVICE;
    c->job_allocs.assign(c->allocs.begin() + first, c->allocs.end());
    c->njobs = njobs;
    return PWR_OK;
}

static void free_jobs(pwr_ctx *c)
{
    for (void *p : c->job_allocs) dfree(c, p);
    c->job_allocs.clear();
    c->jb = JobBufs{};
    c->d_jobrows = nullptr;
    c->njobs = 0;
}

// Build the device state from the host code matrix.  Requires canonical rows.
static int upload(pwr_ctx *c)
{
    if (c->on_device) return PWR_OK;
    const int T = c->T, W0 = c->W_host;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    // drop columns without a base (what the first W_Con, PW:706-763, does) and check the rows
    std::vector<uint32_t> w((size_t)W0 * 6, 0);
    std::vector<long long> rowoff(T + 1, 0);
    c->rowlen.assign(T, 0);
    {
        // (row-parallel: per-thread symbol counts per column -- 7 counters, "not b" tallies derived at the end)
        const unsigned nth = par_threads(T);
        std::vector<std::vector<uint32_t>> cnt(nth, std::vector<uint32_t>((size_t)W0 * 6, 0));   // counts of symbols 0..5 per column
        std::vector<int> errs(nth, 0);
        par_rows(T, [&](int r0, int r1, int t) {
            uint32_t *ct = cnt[t].data();
            for (int r = r0; r < r1; ++r) {
                const unsigned char *row = &c->text[(size_t)r * W0];
                int L = 0;
                for (int i = 0; i < W0; ++i) {
                    const int s = row[i];
                    L += s < 4;
                    ct[(size_t)i * 6 + s] += 1;
                }
                // every maximal run of non-blank cells must be a segment base..base (what EntAlGapper, PW:459-645, leaves behind)
                for (int i = 0; i < W0; ++i) {
                    if (row[i] == 5) continue;
                    int j = i;
                    while (j + 1 < W0 && row[j + 1] != 5) ++j;
                    if (row[i] >= 4 || row[j] >= 4) { errs[t] = PWR_ERR_UNSUPPORTED; return; }
                    i = j;
                }
                if (L > PWR_MAX_SEQ_LENGTH) { errs[t] = PWR_ERR_RANGE; return; }   // PW:675-680
                c->rowlen[r] = L;
            }
        });
        for (int e : errs) if (e == PWR_ERR_UNSUPPORTED) return e;
        for (int e : errs) if (e) return e;
        // w[b] = rows non-blank and != b (PW:165-222) = (non-blank rows) - (rows with symbol b)
        for (int i = 0; i < W0; ++i) {
            uint32_t n[6] = {0, 0, 0, 0, 0, 0};
            for (unsigned t = 0; t < nth; ++t) for (int b = 0; b < 6; ++b) n[b] += cnt[t][(size_t)i * 6 + b];
            const uint32_t cov = n[0] + n[1] + n[2] + n[3] + n[4];
            for (int b = 0; b < 5; ++b) w[(size_t)i * 6 + b] = cov - n[b];
            w[(size_t)i * 6 + 5] = cov;
        }
        for (int r = 0; r < T; ++r) rowoff[r + 1] = rowoff[r] + c->rowlen[r];
    }
    c->sumL = rowoff[T];
    c->Lmax = 0;
    for (int r = 0; r < T; ++r) c->Lmax = std::max(c->Lmax, c->rowlen[r]);
    std::vector<int> colidx(W0, -1);
    int W = 0;
    for (int i = 0; i < W0; ++i) if (w[(size_t)i * 6 + 4] != 0) colidx[i] = W++;
    if (W == 0) W = 0;
    std::vector<Tally> tal(std::max(W, 1));
    memset(tal.data(), 0, sizeof(Tally) * tal.size());
    for (int i = 0; i < W0; ++i)
        if (colidx[i] >= 0) for (int b = 0; b < 6; ++b) tal[colidx[i]].w[b] = w[(size_t)i * 6 + b];
    std::vector<uint8_t> seq(std::max<long long>(c->sumL, 1));
    std::vector<int> pos(std::max<long long>(c->sumL, 1));
    std::vector<long long> brkoff(T + 1, 0);
    std::vector<int> brkx, nbrk(T, 0);
    {
        // (row-parallel; the breaks and the segment ends a thread finds are merged in row order afterwards)
        const unsigned nth = par_threads(T);
        std::vector<std::vector<int>> tb(nth), tend(nth);       // per thread: break indices of its rows in order; columns that end a segment
        par_rows(T, [&](int r0, int r1, int t) {
            std::vector<int> &bx = tb[t], &en = tend[t];
            for (int r = r0; r < r1; ++r) {
                const unsigned char *row = &c->text[(size_t)r * W0];
                long long o = rowoff[r];
                int last = -1;
                const size_t b0 = bx.size();
                for (int i = 0; i < W0; ++i) {
                    if (row[i] < 4) { seq[o] = row[i]; pos[o] = colidx[i]; last = colidx[i]; ++o; }
                    else if (row[i] == 5 && last >= 0 && i > 0 && row[i - 1] != 5) {
                        // a segment ends in the column before: an inner end if more bases follow (settled below)
                        bx.push_back((int)(o - rowoff[r]) - 1);
                    }
                }
                // the blank run after the row's LAST base is its margin, not a break
                while (bx.size() > b0 && bx.back() == c->rowlen[r] - 1) bx.pop_back();
                nbrk[r] = (int)(bx.size() - b0);
                for (size_t q = b0; q < bx.size(); ++q) en.push_back(pos[rowoff[r] + bx[q]]);
                if (last >= 0) en.push_back(last);
            }
        });
        for (unsigned t = 0; t < nth; ++t) {
            brkx.insert(brkx.end(), tb[t].begin(), tb[t].end());
            for (int col : tend[t]) tal[col].endcnt += 1;
        }
        long long acc = 0;
        for (int r = 0; r < T; ++r) { brkoff[r] = acc; acc += nbrk[r]; }
    }
    brkoff[T] = (long long)brkx.size();
    // capacities
    DState &st = c->st;
    st = DState{};
    st.T = T; st.B = c->B; st.H = c->H; st.Lmax = c->Lmax;
    st.colcap = ((c->cap_slack ? 2 * W + 2 * c->Lmax + c->cap_slack : W + c->Lmax + 128) + 15) & ~15;   // (a multiple of 16: the per-job mark arrays are read 8 bytes at a time)
    st.slotcap = st.colcap;
    int rc;
    Hdr hdr{};
    hdr.W = W; hdr.nslots = W; hdr.nfree = 0; hdr.cur = 0; hdr.agree = 0; hdr.noseg_row = -1;
    {
        const long long hi = std::min<long long>((long long)c->B * c->warm_pct / 100 + 2, 1 << 20);
        const long long lo = std::min<long long>(hi, (long long)c->B * c->warm_min_pct / 100 + 2);
        hdr.warm_hi = (int)hi; hdr.warm_lo = (int)lo;
        hdr.warm_cur = (int)std::max(lo, std::min(hi, (long long)c->B * 140 / 100));
        hdr.warm_step = (c->warm_adapt && c->src_start) ? std::max(1, (int)((long long)c->B * c->warm_down_pm / 1000)) : 0;
        hdr.warm_up = std::max(1, (int)((long long)c->B * c->warm_up_pm / 1000));
    }
    long long *d_rowoff; int *d_rowlen; uint8_t *d_seq;
    if ((rc = dmalloc(c, &st.hdr, 1))) return rc;
    if ((rc = dmalloc(c, &st.bplan, BPLAN_WORDS))) return rc;
    HIPC(hipMemset(st.bplan, 0, sizeof(int) * BPLAN_WORDS));
    if ((rc = dmalloc(c, &d_rowoff, T + 1))) return rc;
    if ((rc = dmalloc(c, &d_rowlen, T))) return rc;
    if ((rc = dmalloc(c, &d_seq, seq.size()))) return rc;
    if ((rc = dmalloc(c, &st.pos, pos.size()))) return rc;
    if ((rc = dmalloc(c, &st.tally, st.slotcap))) return rc;
    if ((rc = dmalloc(c, &st.order0, st.colcap))) return rc;
    if ((rc = dmalloc(c, &st.order1, st.colcap))) return rc;
    if ((rc = dmalloc(c, &st.rank, st.slotcap))) return rc;
    if ((rc = dmalloc(c, &st.freelist, st.slotcap))) return rc;
    if ((rc = dmalloc(c, &st.inscnt, st.colcap))) return rc;
    if ((rc = dmalloc(c, &st.newidx, st.colcap))) return rc;
    if ((rc = dmalloc(c, &c->d_score, 1))) return rc;
    st.rowoff = d_rowoff; st.rowlen = d_rowlen; st.seq = d_seq;
    {
        long long *d_brkoff; int *d_brkx;
        if ((rc = dmalloc(c, &d_brkoff, T + 1))) return rc;
        if ((rc = dmalloc(c, &d_brkx, brkx.size()))) return rc;
        if ((rc = dmalloc(c, &st.nbrk, T))) return rc;
        if ((rc = dmalloc(c, &st.hard, T))) return rc;
        HIPC(hipMemset(st.hard, 0, sizeof(int) * T));
        HIPC(hipMemcpy(d_brkoff, brkoff.data(), sizeof(long long) * (T + 1), hipMemcpyHostToDevice));
        if (!brkx.empty()) HIPC(hipMemcpy(d_brkx, brkx.data(), sizeof(int) * brkx.size(), hipMemcpyHostToDevice));
        HIPC(hipMemcpy(st.nbrk, nbrk.data(), sizeof(int) * T, hipMemcpyHostToDevice));
        st.brkoff = d_brkoff; st.brkx = d_brkx;
    }
    std::vector<int> ident(std::max(W, 1));
    for (int i = 0; i < W; ++i) ident[i] = i;
    HIPC(hipMemcpy(st.hdr, &hdr, sizeof hdr, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_rowoff, rowoff.data(), sizeof(long long) * (T + 1), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_rowlen, c->rowlen.data(), sizeof(int) * T, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_seq, seq.data(), seq.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(st.pos, pos.data(), sizeof(int) * pos.size(), hipMemcpyHostToDevice));
    HIPC(hipMemset(st.tally, 0, sizeof(Tally) * st.slotcap));
    HIPC(hipMemcpy(st.tally, tal.data(), sizeof(Tally) * W, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(st.order0, ident.data(), sizeof(int) * W, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(st.rank, ident.data(), sizeof(int) * W, hipMemcpyHostToDevice));
    HIPC(hipMemset(st.inscnt, 0, sizeof(int) * st.colcap));
    {
        c->ids.clear(); c->pos_lo.assign(T + 1, 0);
        for (int r = 0; r < T; ++r) { c->pos_lo[r] = (int)c->ids.size(); if (c->rowlen[r] > 0) c->ids.push_back(r); }
        c->pos_lo[T] = (int)c->ids.size();
        if ((rc = dmalloc(c, &c->d_rowids, std::max<size_t>(1, c->ids.size())))) return rc;
        if (!c->ids.empty()) HIPC(hipMemcpy(c->d_rowids, c->ids.data(), sizeof(int) * c->ids.size(), hipMemcpyHostToDevice));
    }
    HIPC(hipStreamCreate(&c->stream));
    if ((rc = alloc_jobs(c, std::max(1, c->window)))) return rc;
    c->on_device = true;
    std::vector<unsigned char>().swap(c->text);
    c->W_host = 0;
    return PWR_OK;
}

static int read_hdr(pwr_ctx *c, Hdr *h)
{
    // one async copy into pinned memory + one stream wait: the only host round trip of a batch
    if (!c->h_hdr) {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(Hdr), hipHostMallocDefault) != hipSuccess) return PWR_ERR_NOMEM;
        c->h_hdr = p;
    }
    HIPC(hipMemcpyAsync(c->h_hdr, c->st.hdr, sizeof(Hdr), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    memcpy(h, c->h_hdr, sizeof(Hdr));
    return PWR_OK;
}

// grow a device array, keeping its first `keep` elements
template <typename T>
static int regrow(pwr_ctx *c, T **p, size_t keep, size_t ncap)
{
    T *q;
    int rc = dmalloc(c, &q, ncap);
    if (rc) return rc;
    if (hipMemset(q, 0, ncap * sizeof(T)) != hipSuccess) return PWR_ERR_DEVICE;
    if (keep && hipMemcpy(q, *p, keep * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) return PWR_ERR_DEVICE;
    dfree(c, *p);
    *p = q;
    return PWR_OK;
}

// A commit found the column arrays too small (Hdr::need_grow): make room for at least `growth` more columns.  The stream
// is idle when this runs.  `ncommitted`: the jobs of the batch that was stopped which committed before the one that did not
// fit -- the row pointer has moved on with them then, and the plan that batch ran by (DState::bplan, offsets from the row
// pointer as it stood) says nothing about the rows that follow: the next batch takes them in order.  (k_commit_finish
// has dropped the plan already; here once more, for every path that goes on after a regrow.)
static int grow_state(pwr_ctx *c, long long growth, int ncommitted)
{
    Hdr h;
    int rc = read_hdr(c, &h);
    if (rc) return rc;
    if (h.status) return h.status;
    c->grows += 1;
    if (ncommitted > 0) c->grows_mid_batch += 1;
    HIPC(hipMemsetAsync(c->st.bplan, 0, sizeof(int), c->stream));                 // (the jump records and Hdr::jumpmask stay: they belong to rows)
    DState &st = c->st;
    const size_t ncap = ((size_t)std::max<long long>(2LL * st.colcap, (long long)std::max(h.W, h.nslots) + 2 * growth + 8192) + 15) & ~(size_t)15;
    const size_t ocol = st.colcap, oslot = st.slotcap;
    if ((rc = regrow(c, &st.tally, oslot, ncap))) return rc;
    if ((rc = regrow(c, &st.order0, ocol, ncap))) return rc;
    if ((rc = regrow(c, &st.order1, ocol, ncap))) return rc;
    if ((rc = regrow(c, &st.rank, oslot, ncap))) return rc;
    if ((rc = regrow(c, &st.freelist, oslot, ncap))) return rc;
    if ((rc = regrow(c, &st.inscnt, 0, ncap))) return rc;
    if ((rc = regrow(c, &st.newidx, 0, ncap))) return rc;
    st.colcap = (int)ncap; st.slotcap = (int)ncap;
    const int nj = c->njobs;
    free_jobs(c);
    if ((rc = alloc_jobs(c, nj))) return rc;
    const int zero = 0;
    HIPC(hipMemcpy(&st.hdr->need_grow, &zero, sizeof(int), hipMemcpyHostToDevice));
    return PWR_OK;
}

static int launch_fill(pwr_ctx *c, int njobs)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // (an event record costs about 6 us on the stream, two of them 3 % of a batch: with "profile" 1 every launch is timed,
    // with "profile" n > 1 every n-th; pwr_stats.fill_launches_timed says how many the sum covers)
    const bool timed = c->profile && (c->stats.fill_launches % (unsigned)c->profile) == 0 && c->ev_used < (size_t)(1 << 16);
    if (timed) {
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t a, b;
            HIPC(hipEventCreate(&a)); HIPC(hipEventCreate(&b));
            c->ev_pool.emplace_back(a, b);
        }
        e0 = c->ev_pool[c->ev_used].first; e1 = c->ev_pool[c->ev_used].second;
        c->ev_used++;
        HIPC(hipEventRecord(e0, c->stream));
    }
    if (c->fill_mode == 4) {
        // one work-group (worker + fetcher wave) per wave of the pipeline; grid.x = 8 keeps the work-groups of a DP
        // on one XCD (work-groups go to the XCDs round-robin by linear id)
        if (++c->fill_epoch >= (1 << 15)) {
            const size_t nmb = (size_t)c->njobs * c->wp_waves * c->jb.gstride;
            HIPC(hipMemsetAsync(c->jb.gmb, 0, nmb * 8, c->stream));
            c->fill_epoch = 1;
        }
        c->jb.tagbase = (unsigned)c->fill_epoch << 17;
        c->jb.njobs_launched = njobs;
        c->jb.stall_test = c->stall_test > 0 ? 1 : 0;
        c->jb.v2_follows = (c->seen_fallback > 0 && c->wp_waves != 17) ? 1 : 0;
        if (c->stall_test > 0) c->stall_test -= 1;
        const int nv = njobs * c->jb.smax;                                 // one slot per (job, segment)
        const dim3 grid(8, c->wp_waves, (nv + 7) / 8);
        const bool wg1 = c->one_wg && c->wp_waves <= 9 && c->B <= 1024 && c->wave_cols != 4;
        if (wg1) {
            // the waves of a segment as one work-group (LDS hand-over); "onewg_lds" bytes of dynamic LDS on top keep other
            // work-groups off the segment's compute unit (experiment: a CU to itself, one wave per SIMD with waves = 4)
            // (wg1 leaves out the two pairs that have no such kernel: 17 waves, and 9 waves with strips of 256 columns)
            const size_t pad = (size_t)c->one_wg_lds;
            with_geometry(c, [&](auto NW, auto C) {
                if constexpr (NW != 17 && !(NW == 9 && C == 4))
                    hipLaunchKernelGGL((k_fill_v3<NW, C, true>), dim3(nv), dim3(NW * 64), pad, c->stream, c->st, c->jb);
            });
        }
        else with_geometry(c, [&](auto NW, auto C) {
            const size_t lds = NW == 5 ? (size_t)c->fill_lds : 0;               // ("fill_lds" is an experiment on the default fill alone)
            hipLaunchKernelGGL((k_fill_v3<NW, C, false>), grid, dim3(128), lds, c->stream, c->st, c->jb);
        });
        c->jb.stall_test = 0;
        if (c->jb.smax > 1 && c->jb.seg_rows > 0 && !c->jb.check_in_trace)
            hipLaunchKernelGGL(k_seg_check, dim3(njobs, c->jb.smax - 1), dim3(256), 0, c->stream, c->st, c->jb);
    }
    // k_fill_v2: the fill of its own right (option fill = 3), or the stand-in behind k_fill_v3 that only runs while
    // Hdr::fallback > 0, i.e. after a k_fill_v3 job gave up waiting for a neighbour work-group
    c->jb.gate_v2 = c->fill_mode == 4 ? 1 : 0;
    if (c->fill_mode == 3) c->jb.v2_follows = 1;
    if (c->fill_mode == 3 || (c->fill_mode == 4 && c->jb.v2_follows)) {
        with_geometry(c, [&](auto NW, auto C) {
            if constexpr (NW != 17)                                             // (17 x 64 threads do not fit one work-group: settle_geometry, v2_follows)
                hipLaunchKernelGGL((k_fill_v2<NW, C>), dim3(njobs), dim3(NW * 64), 0, c->stream, c->st, c->jb);
        });
    } else if (c->fill_mode != 4) return PWR_ERR_ARG;
    HIPC(hipGetLastError());
    if (timed) { HIPC(hipEventRecord(e1, c->stream)); c->stats.fill_launches_timed += 1; }
    c->stats.fill_launches += 1;
    return PWR_OK;
}

static int drain_events(pwr_ctx *c)
{
    if (!c->ev_used) return PWR_OK;
    HIPC(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->ev_used; ++i) {
        float ms = 0;
        HIPC(hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second));
        c->stats.fill_ms += ms;
    }
    c->ev_used = 0;
    return PWR_OK;
}

static int ensure_device(pwr_ctx *c)
{
    if (c->on_device) { if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE; return PWR_OK; }
    int rc = upload(c);
    if (rc) { free_device(c); return rc; }
    return PWR_OK;
}

static void stats_from_hdr(pwr_ctx *c, const Hdr &h)
{
    c->stats.cells_computed = h.cells_computed;
    c->stats.cells_reference = h.cells_reference;
    c->stats.rows_changed = h.rows_changed;
    c->stats.batches = h.batches;
    c->stats.rows_committed = h.rows_committed;
    c->stats.rows_recomputed = h.rows_recomputed;
    c->stats.rows_wide = h.rows_wide;
    c->stats.stalls = h.stalls;
    c->stats.rows_ahead = h.rows_ahead;
    c->stats.seg_jobs = h.seg_jobs; c->stats.segs = h.segs; c->stats.seg_fails = h.seg_fails;
    c->stats.rows_jumped = h.rows_jumped;
    for (int i = 0; i < 4; ++i) c->stats.reject_reason[i] = h.fail_reason[i];
}

static int check_status(pwr_ctx *c)
{
    Hdr h;
    int rc = read_hdr(c, &h);
    if (rc) return rc;
    stats_from_hdr(c, h);
    return h.status;
}

// One speculative batch, enqueued without waiting: the rows rowids[next_row ...] (Hdr, at most `window` of them) are
// gathered from the committed state, filled and traced side by side, then committed in row order by one work-group that stops
// at the first row whose inputs an earlier commit of this batch has changed, moves next_row on and sizes the next batch.
static int enqueue_front(pwr_ctx *c)
{
    const int n = c->window;
    int rc;
    c->jb.gather_tag = ++c->gather_tag;
    c->jb.rowids = c->d_rowids;
    c->jb.f64_follows = (c->seen_need64 > 0 || c->force64) ? 1 : 0;
    hipLaunchKernelGGL(k_gather_a, dim3(n, GATHER_G), dim3(GATHER_NT), 0, c->stream, c->st, c->jb, c->d_rowids);
    hipLaunchKernelGGL(k_gather_c, dim3(n, GATHER_G + 1), dim3(GATHER_NT), 0, c->stream, c->st, c->jb);
    // (the check of the segments' starts rides in k_trace_blk's launch when that is the traceback of this batch)
    c->jb.trace_ny = (c->jb.Lmax / TB_C + TB_W) / TB_W;
    c->jb.check_in_trace = (c->check_in_trace && c->fill_mode == 4 && c->par_trace == 2 && c->st.colcap < TB_MAXCOL && c->jb.smax > 1 && c->jb.seg_rows > 0) ? 1 : 0;
    if ((rc = launch_fill(c, n))) return rc;
    if (c->jb.f64_follows) hipLaunchKernelGGL(k_fill64, dim3(n), dim3(F64_NT), 0, c->stream, c->st, c->jb);   // jobs the gather flagged wide
    if (c->par_trace) {
        if (++c->trace_epoch >= (1 << 14)) { HIPC(hipMemsetAsync(c->jb.gtr, 0, (size_t)c->njobs * c->jb.trk * 8, c->stream)); c->trace_epoch = 1; }
        c->jb.trace_tag = (unsigned)c->trace_epoch;
        c->jb.trace_blk = (c->par_trace == 2 && c->st.colcap < TB_MAXCOL) ? 1 : 0;
        c->jb.trace_prior = c->trace_prior;
        if (c->jb.trace_blk) hipLaunchKernelGGL(k_trace_blk, dim3(n, c->jb.trace_ny + (c->jb.check_in_trace ? c->jb.smax - 1 : 0)), dim3(TB_W * 64), 0, c->stream, c->st, c->jb);
        else hipLaunchKernelGGL(k_trace_par, dim3(n, TRK / TRW), dim3(TRW * 64), 0, c->stream, c->st, c->jb);
    }
    else { c->jb.trace_blk = 0; hipLaunchKernelGGL(k_trace_wp, dim3(n), dim3(64), 0, c->stream, c->st, c->jb); }
    HIPC(hipGetLastError());
    return PWR_OK;
}

// the commit of a batch: what changes (per job and share), who commits and the changes themselves, the renumbering and the header
static int enqueue_commit(pwr_ctx *c, Hdr *host_copy, unsigned host_seq)
{
    const int n = c->window;
    hipLaunchKernelGGL(k_commit_scan, dim3(n, CS_G), dim3(COMMIT_NT), 0, c->stream, c->st, c->jb, n);
    hipLaunchKernelGGL(k_commit_finish, dim3(CA_G), dim3(COMMIT_NT), 0, c->stream, c->st, c->jb, n, c->d_rowids, host_copy, host_seq);
    HIPC(hipGetLastError());
    return PWR_OK;
}

static int enqueue_batch(pwr_ctx *c, Hdr *host_copy, unsigned host_seq)
{
    int rc = enqueue_front(c);
    if (rc) return rc;
    return enqueue_commit(c, host_copy, host_seq);
}

#define PWR_INFLIGHT 3             // batches enqueued beyond the last one whose outcome the host has seen
#define PWR_POLL_LIMIT_S 120       // how long the host waits for the header of ONE batch before it gives the context up

// Start a slab: rows [k0, k0 + n), first batch sized like the host did before (the running mean carries over).  (After a
// regrow a slab goes on where it stood instead: the device's row pointer and its mask of rows already committed ahead of
// order stay as they are -- each row is realigned once per round, PW:1695.)
static int slab_init(pwr_ctx *c, int k0, int n)                              // (k0, n: POSITIONS in the list of rows that have bases)
{
    const int kend = k0 + n;
    int nb = (int)(c->batch_ema + 2.6);
    nb = std::max(1, std::min(nb, std::min(c->window, n)));
    for (int j = 1; j < nb; ++j)
        if (c->rowlen[c->ids[k0 + j]] > c->rowlen[c->ids[k0]] + (int)((long long)c->rowlen[c->ids[k0]] * c->spec_len / 100) + 64) { nb = j; break; }
    const float ema0 = (float)c->batch_ema;
    struct { int next_row, row_end, nb, need_grow, window; } init = {k0, kend, nb, 0, c->window};
    static_assert(sizeof(init) == offsetof(Hdr, fallback) - offsetof(Hdr, next_row), "slab fields of Hdr");
    HIPC(hipMemcpyAsync(&c->st.hdr->ema, &ema0, sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(&c->st.hdr->speclen, &c->spec_len, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(&c->st.hdr->next_row, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(&c->st.hdr->ahead, 0, sizeof(unsigned long long), c->stream));
    HIPC(hipMemsetAsync(c->st.bplan, 0, sizeof(int), c->stream));                 // (the slab's first batch: the next rows in order)
    HIPC(hipMemsetAsync(&c->st.hdr->jumpmask, 0, sizeof(unsigned long long), c->stream));
    HIPC(hipStreamSynchronize(c->stream));                                     // (init lives on the stack)
    return PWR_OK;
}

// Rows k0 .. k0+n-1 in input order (a slab of the k loop, PW:1695-1737), speculative batches inside the slab only.  The
// device sequences the rows itself (Hdr::next_row); the host keeps PWR_INFLIGHT batches queued and looks at a copy of the
// header that trails by that many batches, so no launch waits for a round trip.  Batches enqueued after the slab's last row
// was committed find nothing to do.
static int realign_positions(pwr_ctx *c, int k0, int n, bool resume = false)   // (k0, n: positions in the list of rows that have bases)
{
    if (!c->h_ring) {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(Hdr) * PWR_INFLIGHT, hipHostMallocDefault) != hipSuccess) return PWR_ERR_NOMEM;
        c->h_ring = p;
        memset(p, 0, sizeof(Hdr) * PWR_INFLIGHT);                              // (sequence numbers start at 1)
    }
    Hdr *ring = static_cast<Hdr *>(c->h_ring);
    unsigned seqs[PWR_INFLIGHT] = {};
    const int kend = k0 + n;
    int rc;
    c->split_rank = 0; c->split_world = 1; c->jb.split_rank = 0; c->jb.split_world = 1;   // (every job of a batch is this context's)
    if (!resume && (rc = slab_init(c, k0, n))) return rc;
    long long issued = 0, looked = 0;                                          // batches enqueued / batches whose outcome the host has seen
    long long most = n;                                                        // every batch with rows left commits at least one ...
    while (true) {
        while (issued < most && issued - looked < PWR_INFLIGHT) {
            const int slot = (int)(issued % PWR_INFLIGHT);
            const auto t_e = std::chrono::steady_clock::now();
            if ((rc = enqueue_batch(c, &ring[slot], ++c->host_seq))) return rc;   // (its commit kernel leaves the header in ring[slot], this number last)
            c->host_enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_e).count();
            seqs[slot] = c->host_seq;
            ++issued;
        }
        if (looked == issued) {                                                // rows left although every batch commits one: cannot happen
            (void)hipStreamSynchronize(c->stream);
            fprintf(stderr, "pwr: %lld batches issued for %d rows and rows are left (host guard, not the traceback's error)\n", issued, n);
            return PWR_ERR_INTERNAL;
        }
        const int slot = (int)(looked % PWR_INFLIGHT);
        {
            // wait for that batch's header: poll the sequence number (pinned memory), look at the stream now and then in case
            // it has died
            volatile unsigned *sq = &ring[slot].seq;
            const auto t_w = std::chrono::steady_clock::now();
            std::chrono::steady_clock::time_point t_wait{};
            for (unsigned long long spin = 1; *sq != seqs[slot]; ++spin) {
                if ((spin & 0xfffffull) == 0) {
                    if (hipStreamQuery(c->stream) == hipSuccess && *sq != seqs[slot]) {
                        // the stream is idle and the header never came: a launch failed
                        hipError_t e = hipGetLastError();
                        fprintf(stderr, "pwr: a batch ended without its header (%s)\n", hipGetErrorString(e));
                        return PWR_ERR_DEVICE;
                    }
                    // a batch takes a fraction of a millisecond, a wave that waits in vain for its neighbour gives up after 0.2 s
                    // (V3_TIMEOUT_TICKS) and the stand-in kernel takes milliseconds: a header that has not come after PWR_POLL_LIMIT_S
                    // seconds never will (a kernel that does not end).  Say which one, and return instead of spinning for ever.
                    const auto now = std::chrono::steady_clock::now();
                    if (t_wait == std::chrono::steady_clock::time_point{}) t_wait = now;
                    else if (std::chrono::duration<double>(now - t_wait).count() > PWR_POLL_LIMIT_S) {
                        fprintf(stderr, "pwr: no header from batch %lld of the slab (sequence %u) after %d s: a kernel of it does not end\n", looked, seqs[slot], PWR_POLL_LIMIT_S);
                        return PWR_ERR_STALL;
                    }
                    std::this_thread::yield();
                }
#if !defined(__HIP_DEVICE_COMPILE__)
                __builtin_ia32_pause();
#endif
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            c->host_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_w).count();
        }
        const Hdr h = ring[slot];
        ++looked;
        c->seen_fallback = h.fallback; c->seen_need64 = h.need64;
        if (h.status) { (void)hipStreamSynchronize(c->stream); return h.status; }
        if (h.need_grow) {
            // the batches queued behind this one do nothing while the flag is up
            HIPC(hipStreamSynchronize(c->stream));
            long long growth = 0;
            for (int j = 0; j < c->window && h.next_row + j < kend; ++j) growth += c->rowlen[c->ids[h.next_row + j]];
            if ((rc = grow_state(c, growth, h.ncommitted))) return rc;
            return realign_positions(c, h.next_row, kend - h.next_row, true);
        }
        if (h.next_row >= kend) break;
        if (h.ncommitted == 0 && most < 4LL * n + 256) ++most;                  // ... except one whose first job stalled, failed its segment check, or came without the kernel it needed
    }
    HIPC(hipStreamSynchronize(c->stream));                                     // the no-op batches behind the last real one
    Hdr h;
    if ((rc = read_hdr(c, &h))) return rc;
    c->batch_ema = h.ema;
    c->seen_fallback = h.fallback; c->seen_need64 = h.need64;
    stats_from_hdr(c, h);
    return h.status;
}

// rows k0 .. k0 + n - 1: the rows among them that have bases, a run of the list
static int realign_range(pwr_ctx *c, int k0, int n)
{
    const int p0 = c->pos_lo[k0], pn = c->pos_lo[k0 + n] - p0;
    if (pn == 0) return check_status(c);
    return realign_positions(c, p0, pn);
}

static int realign_row(pwr_ctx *c, int k)
{
    if (!c || k < 0 || k >= c->T) return PWR_ERR_ARG;
    int rc = ensure_device(c);
    if (rc) return rc;
    return realign_range(c, k, 1);
}

static int realign_rows(pwr_ctx *c, int k0, int n)
{
    if (!c || k0 < 0 || n < 0 || k0 > c->T || n > c->T - k0) return PWR_ERR_ARG;
    int rc = ensure_device(c);
    if (rc) return rc;
    if (n == 0) return PWR_OK;
    return realign_range(c, k0, n);
}

static int realign_round(pwr_ctx *c)
{
    if (!c) return PWR_ERR_ARG;
    int rc = ensure_device(c);
    if (rc) return rc;
    return realign_range(c, 0, c->T);                                          // PW:1695: rows in input order
}

// ---------------------------------------------------------------------------------------------
// One round split over the GPUs of a node ("within one MSA").  Every rank is a replica: it holds
// the whole state, gathers every job of a batch and commits every job in row order -- so the replicas stay identical
// without any state ever crossing a link --, but it FILLS and TRACES only its share of the batch (job j belongs to rank
// j % world).  What crosses xGMI per batch is one record per job (new placement + a few words, pwr_split_slot_bytes):
//     pwr_split_begin(ctx, k0, n, rank, world)
//     do { pwr_split_stage(ctx, send);  all_gather(recv, send);  pwr_split_commit(ctx, recv, &left); } while (left > 0);
// `send` = slots_per_rank * slot_bytes of DEVICE memory, `recv` = world times that, ranks in order (what RCCL's
// all-gather produces).  The collective is the caller's (torch.distributed / RCCL): this library links no communication
// library.  The results are those of pwr_realign_rows(k0, n) on one GPU, bit for bit.
// ---------------------------------------------------------------------------------------------
static int split_begin(pwr_ctx *c, int k0, int n, int rank, int world)
{
    if (!c || k0 < 0 || n < 0 || k0 > c->T || n > c->T - k0 || world < 1 || rank < 0 || rank >= world) return PWR_ERR_ARG;
    int rc = ensure_device(c);
    if (rc) return rc;
    c->split_rank = rank; c->split_world = world;
    c->jb.split_rank = rank; c->jb.split_world = world;
    c->split_k0 = c->pos_lo[k0]; c->split_kend = c->pos_lo[k0 + n];             // (positions in the list of rows that have bases)
    if (n == 0) return PWR_OK;
    return slab_init(c, c->split_k0, c->split_kend - c->split_k0);
}

static int split_slots(pwr_ctx *c, size_t *slot_bytes, int *slots_per_rank)
{
    if (!c || !slot_bytes || !slots_per_rank) return PWR_ERR_ARG;
    int rc = ensure_device(c);
    if (rc) return rc;
    *slot_bytes = split_slot_bytes(c->jb.Lmax, c->jb.trk);
    *slots_per_rank = (c->window + c->split_world - 1) / c->split_world;
    return PWR_OK;
}

static int split_stage(pwr_ctx *c, void *send_dev)
{
    if (!c || !send_dev || !c->on_device) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    int rc = enqueue_front(c);
    if (rc) return rc;
    hipLaunchKernelGGL(k_split_export, dim3(c->window), dim3(256), 0, c->stream, c->jb, c->window, static_cast<unsigned char *>(send_dev));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(c->stream));                                     // the caller's collective runs on a stream of its own
    return PWR_OK;
}

static int split_commit(pwr_ctx *c, const void *recv_dev, int *rows_left)
{
    if (!c || !recv_dev || !rows_left || !c->on_device) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (c->split_world > 1)
        hipLaunchKernelGGL(k_split_import, dim3(c->window), dim3(256), 0, c->stream, c->st, c->jb, c->window, static_cast<const unsigned char *>(recv_dev));
    int rc = enqueue_commit(c, static_cast<Hdr *>(nullptr), 0u);
    if (rc) return rc;
    Hdr h;
    if ((rc = read_hdr(c, &h))) return rc;                                     // (waits for the stream)
    c->seen_fallback = h.fallback; c->seen_need64 = h.need64;
    c->batch_ema = h.ema;
    stats_from_hdr(c, h);
    if (h.status) return h.status;
    if (h.need_grow) {
        // every replica finds the same shortage in the same batch and regrows alike; the slab goes on where it stands
        long long growth = 0;
        for (int j = 0; j < c->window && h.next_row + j < c->split_kend; ++j) growth += c->rowlen[c->ids[h.next_row + j]];
        if ((rc = grow_state(c, growth, h.ncommitted))) return rc;
    }
    *rows_left = std::max(0, h.row_end - h.next_row);
    return PWR_OK;
}

static int total_score(pwr_ctx *c, uint64_t *total)
{
    if (!c || !total) return PWR_ERR_ARG;
    if (!c->on_device) {
        // host state (before the first device call): literal PW:864-892 on the code matrix
        const int T = c->T, W = c->W_host;
        const unsigned nth = par_threads(T);
        std::vector<std::vector<uint32_t>> cnt(nth, std::vector<uint32_t>((size_t)W * 6, 0));   // rows with symbol 0..5, per column
        par_rows(T, [&](int r0, int r1, int t) {
            uint32_t *ct = cnt[t].data();
            for (int r = r0; r < r1; ++r)
                for (int i = 0; i < W; ++i) ct[(size_t)i * 6 + c->text[(size_t)r * W + i]] += 1;
        });
        uint64_t tot = 0;
        for (int i = 0; i < W; ++i) {
            uint64_t n[5] = {0, 0, 0, 0, 0};
            for (unsigned t = 0; t < nth; ++t) for (int b = 0; b < 5; ++b) n[b] += cnt[t][(size_t)i * 6 + b];
            const uint64_t cov = n[0] + n[1] + n[2] + n[3] + n[4];
            for (int b = 0; b < 5; ++b) tot += n[b] * (cov - n[b]);          // = (w[5] - w[b]) * w[b] with w[b] = cov - n[b]
        }
        *total = tot;
        return PWR_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    HIPC(hipMemsetAsync(c->d_score, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_score, dim3(256), dim3(256), 0, c->stream, c->st, c->d_score);
    unsigned long long v = 0;
    HIPC(hipMemcpyAsync(&v, c->d_score, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    *total = v;
    return PWR_OK;
}

extern "C" int pwr_dims(pwr_ctx *c, int *rows, int *width)
{
    if (!c) return PWR_ERR_ARG;
    if (rows) *rows = c->T;
    if (width) {
        if (!c->on_device) *width = c->W_host;
        else {
            if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
            Hdr h;
            int rc = read_hdr(c, &h);
            if (rc) return rc;
            *width = h.W;
        }
    }
    return PWR_OK;
}

static int export_rows(pwr_ctx *c, unsigned char *buf, size_t cap)
{
    static const char chars[6] = {'A', 'C', 'G', 'T', '-', ' '};              // PW:1558-1563
    if (!c || !buf) return PWR_ERR_ARG;
    if (!c->on_device) {
        const size_t n = (size_t)c->T * c->W_host;
        if (cap < n) return PWR_ERR_ARG;
        for (size_t i = 0; i < n; ++i) buf[i] = (unsigned char)chars[c->text[i]];
        return PWR_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    Hdr h;
    int rc = read_hdr(c, &h);
    if (rc) return rc;
    const int W = h.W;
    if (cap < (size_t)c->T * W) return PWR_ERR_ARG;
    if (W == 0) return PWR_OK;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->T, ((size_t)512 << 20) / (size_t)W));
    unsigned char *d = nullptr;
    if ((rc = dmalloc(c, &d, (size_t)chunk * W))) return rc;
    for (int r0 = 0; r0 < c->T; r0 += chunk) {
        const int nr = std::min(chunk, c->T - r0);
        hipLaunchKernelGGL(k_export, dim3(nr), dim3(256), 0, c->stream, c->st, d, r0, nr, W, 0);
        HIPC(hipMemcpyAsync(buf + (size_t)r0 * W, d, (size_t)nr * W, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    dfree(c, d);
    return PWR_OK;
}

// MMA_Auslesen (PW:1556-1598) without the caller waiting for it: the image of the FILE -- every row's characters and its
// '\n' -- is made on the device in stream order (so the calls that follow may change the state at once) and copied to
// page-locked host memory on a second stream; pwr_snapshot_wait blocks until it is there.  The 1.8 GB the drop-in rewrites
// after every improving round (PW:1741) leave the critical path this way (pwr_host.c hands the image to a writer thread).
static int snapshot_begin(pwr_ctx *c, pwr_snapshot **out)
{
    if (!c || !out) return PWR_ERR_ARG;
    *out = nullptr;
    if (c->snap_busy) return PWR_ERR_ARG;                                           // one at a time
    int rc = ensure_device(c);
    if (rc) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    Hdr h;
    if ((rc = read_hdr(c, &h))) return rc;
    const int W = h.W;
    const size_t bytes = (size_t)c->T * (size_t)(W + 1);
    if (bytes > c->snap_cap) {
        if (c->snap_dev) { dfree(c, c->snap_dev); c->snap_dev = nullptr; }
        if (c->snap_host) { (void)hipHostFree(c->snap_host); c->snap_host = nullptr; }
        c->snap_cap = 0;
        const size_t cap = bytes + bytes / 16 + 4096;                               // (the width moves a little from round to round)
        if ((rc = dmalloc(c, &c->snap_dev, cap))) return rc;
        void *hp = nullptr;
        if (hipHostMalloc(&hp, cap, hipHostMallocDefault) != hipSuccess) { dfree(c, c->snap_dev); c->snap_dev = nullptr; return PWR_ERR_NOMEM; }
        c->snap_host = (unsigned char *)hp;
        c->snap_cap = cap;
    }
    if (!c->snap_stream) {
        HIPC(hipStreamCreateWithFlags(&c->snap_stream, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&c->snap_taken, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&c->snap_done, hipEventDisableTiming));
    }
    pwr_snapshot *sn = new (std::nothrow) pwr_snapshot{c, c->T, W, bytes};
    if (!sn) return PWR_ERR_NOMEM;
    if (bytes > 0) {
        hipLaunchKernelGGL(k_export, dim3(c->T), dim3(256), 0, c->stream, c->st, c->snap_dev, 0, c->T, W, 1);
        if (hipEventRecord(c->snap_taken, c->stream) != hipSuccess || hipStreamWaitEvent(c->snap_stream, c->snap_taken, 0) != hipSuccess ||
            hipMemcpyAsync(c->snap_host, c->snap_dev, bytes, hipMemcpyDeviceToHost, c->snap_stream) != hipSuccess ||
            hipEventRecord(c->snap_done, c->snap_stream) != hipSuccess) { delete sn; return PWR_ERR_DEVICE; }
    }
    c->snap_busy = true;
    *out = sn;
    return PWR_OK;
}

// (may be called from another thread than the one that drives the context)
extern "C" int pwr_snapshot_wait(pwr_snapshot *sn, const unsigned char **image, size_t *bytes, int *rows, int *width)
{
    if (!sn || !sn->c) return PWR_ERR_ARG;
    if (hipSetDevice(sn->c->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (sn->bytes > 0) HIPC(hipEventSynchronize(sn->c->snap_done));
    if (image) *image = sn->c->snap_host;
    if (bytes) *bytes = sn->bytes;
    if (rows) *rows = sn->rows;
    if (width) *width = sn->width;
    return PWR_OK;
}

extern "C" void pwr_snapshot_free(pwr_snapshot *sn)
{
    if (!sn) return;
    if (sn->c && sn->bytes > 0 && sn->c->snap_done) { (void)hipSetDevice(sn->c->device); (void)hipEventSynchronize(sn->c->snap_done); }
    if (sn->c) sn->c->snap_busy = false;
    delete sn;
}

static int trim_ends(pwr_ctx *c)
{
    if (!c) return PWR_ERR_ARG;
    if (!c->on_device) { host_trim(c); return PWR_OK; }
    // Device state: every row is blank* (base|'-')* blank* with bases at both ends and every
    // column holds a base (the commit compacts), so EntAlGapper cannot change anything
    // (PW:483-507 only fires on a '-' next to a blank or at an MSA edge).
    return PWR_OK;
}

extern "C" int pwr_set_option(pwr_ctx *c, const char *key, long value)
{
    if (!c || !key) return PWR_ERR_ARG;
    const Option *o = find_option(key);
    if (!o || value < o->lo || value > o->hi || (o->host_only && c->on_device)) return PWR_ERR_ARG;
    if (o->nof && std::find(o->of, o->of + o->nof, (int)value) == o->of + o->nof) return PWR_ERR_ARG;
    c->*o->field = (int)value;
    if (o->mirror) c->jb.*o->mirror = (int)value;
    return PWR_OK;
}

extern "C" int pwr_get_option(pwr_ctx *c, const char *key, long *value)
{
    if (!c || !key || !value) return PWR_ERR_ARG;
    if (const Option *o = find_option(key)) { *value = c->*o->field; return PWR_OK; }
    // the read-only keys: what the device header or the host's clocks say
    if (!strcmp(key, "hard_marked") || !strcmp(key, "hard_fills") || !strcmp(key, "hard_refail")) {   // counters of "hard_rows"
        *value = 0;
        if (c->on_device) { Hdr h; int rc = read_hdr(c, &h); if (rc) return rc; *value = (long)(key[5] == 'm' ? h.hard_marked : key[5] == 'f' ? h.hard_fills : h.hard_refail); }
    }
    else if (!strcmp(key, "evrate_x100")) {                                    // columns a commit opens / empties, running mean x 100
        *value = 0;
        if (c->on_device) { Hdr h; int rc = read_hdr(c, &h); if (rc) return rc; *value = (long)(h.evrate * 100.0f); }
    }
    else if (!strcmp(key, "grows")) *value = c->grows;                        // since the context was made
    else if (!strcmp(key, "grows_mid_batch")) *value = c->grows_mid_batch;
    else if (!strcmp(key, "host_enqueue_us")) *value = (long)(c->host_enqueue_s * 1e6);   // since the context was made
    else if (!strcmp(key, "host_wait_us")) *value = (long)(c->host_wait_s * 1e6);
    else if (!strcmp(key, "warm_now")) {                                      // percent of the bandwidth a warm-up covers right now
        if (!c->on_device) *value = c->warm_pct;
        else { Hdr h; int rc = read_hdr(c, &h); if (rc) return rc; *value = h.warm_step > 0 ? (long)(((long long)h.warm_cur * 100 + c->B / 2) / c->B) : c->warm_pct; }
    }
    else return PWR_ERR_ARG;
    return PWR_OK;
}

extern "C" int pwr_get_stats(pwr_ctx *c, pwr_stats *out)
{
    if (!c || !out) return PWR_ERR_ARG;
    if (c->on_device) {
        if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
        int rc = check_status(c);
        if (rc) return rc;
        if ((rc = drain_events(c))) return rc;      // HIP-event durations are read here, outside any timed region
    }
    *out = c->stats;
    return PWR_OK;
}

extern "C" int pwr_reset_stats(pwr_ctx *c)
{
    if (!c) return PWR_ERR_ARG;
    if (c->on_device) {
        if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
        int rc0 = drain_events(c);
        if (rc0) return rc0;
    }
    c->stats = pwr_stats{};
    if (c->on_device) {
        if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
        HIPC(hipStreamSynchronize(c->stream));
        HIPC(hipMemset(&c->st.hdr->cells_computed, 0, 16 * sizeof(unsigned long long)));
        HIPC(hipMemset(&c->st.hdr->rows_jumped, 0, sizeof(unsigned long long)));
    }
    return PWR_OK;
}

// ---- introspection for kernel-level parity tests (tests/ only) ----
extern "C" int pwr_debug_last_job(pwr_ctx *c, int *L, int *entry, int *W, int *way, int *newcol, int cap)
{
    if (!c || !c->on_device) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    HIPC(hipStreamSynchronize(c->stream));
    JobMeta m;
    HIPC(hipMemcpy(&m, c->jb.meta, sizeof m, hipMemcpyDeviceToHost));
    if (L) *L = m.L;
    if (entry) *entry = m.entry;
    if (W) *W = m.W;
    const int n = std::min(cap, m.L);
    if (way && n > 0) HIPC(hipMemcpy(way, c->jb.way, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (newcol && n > 0) HIPC(hipMemcpy(newcol, c->jb.newcol, sizeof(int) * n, hipMemcpyDeviceToHost));
    return PWR_OK;
}

// column ordinals of the bases of row k, left to right (the counterpart of the oracle's pwo_row_columns); returns the
// number of bases or a negative error
static int debug_row_columns(pwr_ctx *c, int k, int *out, int cap)
{
    if (!c || !c->on_device || k < 0 || k >= c->T || !out) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    const int L = c->rowlen[k];
    if (L == 0) return 0;
    int *d = nullptr;
    int rc = dmalloc(c, &d, (size_t)L);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rowcols, dim3(32), dim3(256), 0, c->stream, c->st, k, d);
    std::vector<int> h(L);
    if (hipMemcpyAsync(h.data(), d, sizeof(int) * L, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { dfree(c, d); return PWR_ERR_DEVICE; }
    dfree(c, d);
    memcpy(out, h.data(), sizeof(int) * std::min(L, cap));
    return L;
}

extern "C" int pwr_debug_rounds(pwr_ctx *c)
{
    if (!c || !c->on_device) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return PWR_ERR_DEVICE;
    JobMeta m;
    if (hipMemcpy(&m, c->jb.meta, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return PWR_ERR_DEVICE;
    return m.rounds;
}

// phase timers of commit and trace (dev builds with -DPWR_DIAG): 32 words, 10 ns ticks and counts; reading clears them
extern "C" int pwr_debug_phase_times(pwr_ctx *c, unsigned long long *out)
{
    if (!c || !c->on_device || !out) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(out, c->st.hdr->dbg, sizeof(unsigned long long) * 32, hipMemcpyDeviceToHost));
    HIPC(hipMemset(c->st.hdr->dbg, 0, sizeof(unsigned long long) * 32));
    return PWR_OK;
}

// shader clock the fill kernel of job 0 ran at: delta s_memtime / delta s_memrealtime (100 MHz)
// per-wave counters of the last k_fill_v3 launch's job 0 (dev builds with -DPWR_DIAG): 32 x 8 words
extern "C" int pwr_debug_fill_diag(pwr_ctx *c, unsigned long long *out)
{
    if (!c || !c->on_device || !out) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(out, c->jb.diag, sizeof(unsigned long long) * 32 * 4096, hipMemcpyDeviceToHost));
    return PWR_OK;
}

extern "C" int pwr_debug_fill_clock(pwr_ctx *c, double *mhz, double *fill_us)
{
    if (!c || !c->on_device) return PWR_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return PWR_ERR_DEVICE;
    HIPC(hipStreamSynchronize(c->stream));
    JobMeta m;
    HIPC(hipMemcpy(&m, c->jb.meta, sizeof m, hipMemcpyDeviceToHost));
    if (mhz) *mhz = m.rclk ? 100.0 * (double)m.clk / (double)m.rclk : 0.0;
    if (fill_us) *fill_us = (double)m.rclk / 100.0;
    return PWR_OK;
}

// ---- the entries of the C ABI whose bodies can allocate on the host (vectors and threads over the whole text, the lists of
// device buffers, the event pool): no exception leaves them (abi_guard.h) ----
extern "C" int pwr_create(pwr_ctx **out, int rows, int width, const unsigned char *text, int bandwidth, int device)
{
    return abi_guard([&] { return create(out, rows, width, text, bandwidth, device); });
}
extern "C" int pwr_trim_ends(pwr_ctx *c) { return abi_guard([&] { return trim_ends(c); }); }
extern "C" int pwr_realign_row(pwr_ctx *c, int k) { return abi_guard([&] { return realign_row(c, k); }); }
extern "C" int pwr_realign_rows(pwr_ctx *c, int k0, int n) { return abi_guard([&] { return realign_rows(c, k0, n); }); }
extern "C" int pwr_realign_round(pwr_ctx *c) { return abi_guard([&] { return realign_round(c); }); }
extern "C" int pwr_split_begin(pwr_ctx *c, int k0, int n, int rank, int world) { return abi_guard([&] { return split_begin(c, k0, n, rank, world); }); }
extern "C" int pwr_split_slot_bytes(pwr_ctx *c, size_t *slot_bytes, int *slots_per_rank) { return abi_guard([&] { return split_slots(c, slot_bytes, slots_per_rank); }); }
extern "C" int pwr_split_stage(pwr_ctx *c, void *send_dev) { return abi_guard([&] { return split_stage(c, send_dev); }); }
extern "C" int pwr_split_commit(pwr_ctx *c, const void *recv_dev, int *rows_left) { return abi_guard([&] { return split_commit(c, recv_dev, rows_left); }); }
extern "C" int pwr_total_score(pwr_ctx *c, uint64_t *total) { return abi_guard([&] { return total_score(c, total); }); }
extern "C" int pwr_export_rows(pwr_ctx *c, unsigned char *buf, size_t cap) { return abi_guard([&] { return export_rows(c, buf, cap); }); }
extern "C" int pwr_snapshot_begin(pwr_ctx *c, pwr_snapshot **out) { return abi_guard([&] { return snapshot_begin(c, out); }); }
extern "C" int pwr_debug_row_columns(pwr_ctx *c, int k, int *out, int cap) { return abi_guard([&] { return debug_row_columns(c, k, out, cap); }); }
