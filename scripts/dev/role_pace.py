"""dev (GPU box, a library built with -DPWR_DIAG -DPWR_DIAG_SEG=<s>): which role's DP row sets the pace of k_fill_v3.
usage: role_pace.py <libpwr_diag.so> [workload] [rows...]

A job is filled in its default geometry (5 waves x 4 columns per lane, segments side by side); the waves of segment <s> of
job 0 log every stretch of the fast path: end row, role, rows, time, cycles waited so far.  Whole 16-row groups that follow
their predecessor without a gap (no one-row loop, no change of strip in between) are tallied per wave and role, warm-up and
own rows apart: cycles per row busy, cycles per row waiting for the left neighbour's word.  The role whose rows wait for
nobody and cost the most busy cycles is the one the others follow."""
import ctypes, os, sys
sys.path.insert(0, ".")
from repeatresolver_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from repeatresolver_amd import datagen as dg
from repeatresolver_amd.realigner import PWReAligner
wl = sys.argv[2] if len(sys.argv) > 2 else "tree_default"
ks = [int(v) for v in sys.argv[3:]] or [0, 1, 2, 3]
NW = 5
ROLE = {0: "INTERIOR", 1: "RIGHT", 2: "LEFT", 3: "flags", 4: "INTERIOR as RIGHT"}
rows = [bytes(r) for r in dg.make_msa(wl)]
g = PWReAligner(rows, bandwidth=1000, window=1)
g.trim_ends(); g.total_score()
lib = _lib.load()
lib.pwr_debug_fill_diag.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
buf = (ctypes.c_uint64 * (32 * 4096))()
tot = {}                                                   # (warm, role) -> [rows, busy cycles, waited cycles, groups, groups that waited]
per_wave = {}
for k in ks:
    g.realign_row(k)
    mhz, us = g.debug_fill_clock()
    lib.pwr_debug_fill_diag(g._h, buf)
    st = g.stats()
    print(f"row {k}: fill {us:.1f} us, clock {mhz:.0f} MHz, segments so far {st['segs']}, failed checks {st['seg_fails']}")
    for w in range(NW):
        d = buf[w * 4096:(w + 1) * 4096]
        L, cyc = d[7], d[0]
        n = min(d[12], 1270)
        print(f"  wave {w}: segment of {L} rows, {cyc} cycles ({cyc / max(L, 1):.0f} per row), waiting {100 * (d[1] + d[2] + d[3]) / max(cyc, 1):.1f} % "
              f"(mid-row {100 * d[1] / max(cyc, 1):.1f}, strip take-over {100 * d[2] / max(cyc, 1):.1f}, run entry {100 * d[3] / max(cyc, 1):.1f})")
        px = pt = pw = None
        for i in range(n):
            xc, t, wt = d[256 + 3 * i], d[257 + 3 * i], d[258 + 3 * i]
            x, cls, nr = xc & 0xffffffff, (xc >> 32) & 0xff, xc >> 40
            if px is not None and nr == 16 and x - 16 == px and t > pt:
                cycles = (t - pt) * 10e-9 * mhz * 1e6           # 100 MHz ticks -> shader clocks
                for key in ((cls >> 4, cls & 15), (w, cls >> 4, cls & 15)):
                    e = (tot if len(key) == 2 else per_wave).setdefault(key, [0, 0.0, 0.0, 0, 0])
                    e[0] += 16; e[1] += cycles - (wt - pw); e[2] += wt - pw; e[3] += 1; e[4] += 1 if wt > pw else 0
            px, pt, pw = x, t, wt
print("whole groups that follow their predecessor directly, all waves and rows above:")
for (warm, role), e in sorted(tot.items()):
    print(f"  {'warm-up' if warm else 'own    '} {ROLE.get(role, role):18s} {e[0]:6d} rows: busy {e[1] / e[0]:6.0f} cycles per row, waiting {e[2] / e[0]:6.0f} "
          f"({100 * e[2] / (e[1] + e[2]):4.1f} % of the time; {e[4]} of {e[3]} groups waited at all)")
print("per wave:")
for (w, warm, role), e in sorted(per_wave.items()):
    print(f"  wave {w} {'warm-up' if warm else 'own    '} {ROLE.get(role, role):18s} {e[0]:6d} rows: busy {e[1] / e[0]:6.0f}, waiting {e[2] / e[0]:6.0f} cycles per row")
g.close()
