"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

A literal restatement, in plain Python and numpy, of the part of the reference's RepeatResolver.c ("RR:") that
include/pgr.h covers: Einlesen (RR:293-429), the MaxCorrs slice (RR:609-646), the preparation in main() (RR:3977-4014),
Cliquer with TheBestUpdater's insertion (RR:1156-1240), Sizes (RR:1650), Dropoff_Cutoff (RR:1460-1522), CliqueGroup
(RR:976-1008) and CliqueCoverage (RR:1064-1096).

PINNED to the unmodified reference program text, linked with a stand-in for its three GSL functions (oracle/gsl_standin.c;
not a GSL-linked binary): fed the reference's own MaxCorrs values, this checker and tests/sd_checker.py reproduce both label
files the reference writes, byte for byte (tests/test_rr_reference.py).  The reference writes none of the intermediate
arrays (cliques, sizes, groups): for those this restatement stays the yardstick.  The only floating point here is the hypergeometric tail, taken from mco_hyper_Q of oracle/libmcoracle.so -- the restatement that
tests/test_mc_oracle.py pins against scipy and exact rationals -- followed by one log10.  Row sets are kept as 0/1
matrices (row r = the r-th kept row), so every count is an exact integer product."""
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXCLIQUE = 30                                                      # RR:4021
_CODE = {ord(c): k for k, c in enumerate("acgt-")}
_CODE.update({ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("_"): 4})

_mco = None


def mco():
    """oracle/libmcoracle.so through ctypes (built by `make -C oracle port`)"""
    global _mco
    if _mco is None:
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True, stdout=subprocess.DEVNULL)
        lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libmcoracle.so"))
        lib.mco_hyper_Q.restype = ctypes.c_double
        lib.mco_hyper_Q.argtypes = [ctypes.c_uint] * 4
        lib.mco_maxcorrs.restype = ctypes.c_int
        lib.mco_maxcorrs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        _mco = lib
    return _mco


def mco_maxcorrs(rows, mincov):
    out = np.zeros(len(rows[0]) * 5)
    assert mco().mco_maxcorrs(len(rows), len(rows[0]), b"".join(rows), mincov, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return out


def read_window(rows, von=None, bis=None):
    """Einlesen: (kept per row, von, bis, codes[kept rows, width])"""
    if von is None and bis is None:
        von, bis = 0, 1500000                                      # RR:3948-3952
    kept, sig = [], []
    for line in rows:
        siglength = len(line)
        if bis > siglength - 1:
            bis = siglength - 1                                    # RR:328
        if line[von] != 32 and line[bis] != 32:                    # RR:330
            kept.append(True)
            sig.append([_CODE.get(ch, 5) for ch in line[von:bis + 1]])
        else:
            kept.append(False)
    codes = np.array(sig, dtype=np.uint8).reshape(len(sig), bis + 1 - von)
    return np.array(kept, dtype=bool), von, bis, codes


def pack(member):
    """0/1 matrix [n, kept rows] -> uint64 [n, sc], sc = kept / 64 + 1 (RR:375), bit r % 64 of word r / 64 = row r"""
    n, T = member.shape
    sc = T // 64 + 1
    out = np.zeros((n, sc), dtype=np.uint64)
    for r in range(T):
        out[:, r // 64] |= member[:, r].astype(np.uint64) << np.uint64(r % 64)
    return out


def default_cutoff(cutoff, width):
    if cutoff < 0.1:
        cutoff = -1.0 * math.log10(1.0 / (width * 5.0))            # RR:3977
    return cutoff


def restrict_coverage(coverage, maxcorrs):
    maxcov = 0
    for c in coverage:
        if c > maxcov:
            maxcov = int(c)
    for i in range(len(maxcorrs)):
        if int(coverage[i // 5]) * 10 < maxcov * 9:                # RR:4013
            maxcorrs[i] = 0.0
    return maxcov


def the_best_updater(clique, best, maxclique, i, Z):
    """RR:1156-1176, line by line"""
    if best[maxclique - 1] >= Z:
        return
    ii = maxclique - 1
    while best[ii] < Z and ii > 0:
        ii -= 1
    ii += 1
    for j in range(maxclique - 1, ii, -1):
        best[j] = best[j - 1]
        clique[j] = clique[j - 1]
    best[ii] = Z
    clique[ii] = i


class Window:
    """The state after Einlesen and the preparation in main()"""

    def __init__(self, rows, maxcorrs_full, von=None, bis=None, cov=30, cutoff=0.0):
        self.kept, self.von, self.bis, codes = read_window(rows, von, bis)
        self.T, self.w = codes.shape                               # signumber, siglength
        self.V = self.w * 5
        self.G = np.zeros((self.V, self.T), dtype=np.int64)        # Groups as 0/1 rows
        for k in range(5):
            self.G[k::5] = (codes == k).T
        self.LC = (codes < 5).T.astype(np.int64)                   # LocalCoverage
        self.coverage = self.LC.sum(axis=1)
        self.gsize = self.G.sum(axis=1)
        full = np.asarray(maxcorrs_full, dtype=np.float64)
        self.maxcorrs = np.array([full[i] for i in range(len(full)) if self.von <= i // 5 <= self.bis])   # RR:631
        assert len(self.maxcorrs) == self.V
        self.cutoff = default_cutoff(cutoff, self.w)
        self.maxcov = restrict_coverage(self.coverage, self.maxcorrs)
        self.mincov = cov
        self.greedy = self.cutoff                                  # RR:4017
        self.significant = [i for i in range(self.V) if self.maxcorrs[i] > self.cutoff]

    # RR:472-488 from exact counts
    def significance(self, schnitt, cov, gr1, gr2, size1, size2):
        if gr1 == 0 or gr2 == 0:
            return 0.0
        q = mco().mco_hyper_Q(schnitt - 1, gr2, cov - gr2, gr1)   # RR:451
        Z = -1.0 * math.log10(q) if q > 0.0 else math.inf
        if math.isinf(Z) or Z > 99:
            Z = 99.0
        if math.isinf(Z) or Z > 98.0:
            s = float(schnitt)                                     # F_beta(Group1, Group2, 1.0), RR:432-447
            F = (1.0 + 1.0) * s
            F = 0.0 if F < 0.0001 else F / ((1 + 1.0 * 1.0) * s + (1.0 * 1.0 * float(size1 - schnitt)) + float(size2 - schnitt))
            Z = 97.90 + F
        return Z

    def cliquer(self, a):
        """RR:1179-1240.  Returns (Clique[31], candidates): candidates = (Z, i) of every i that reached RR:1216."""
        maxclique, greedy = MAXCLIQUE, self.greedy
        clique = [a] + [None] * maxclique                          # unfilled slots: uninitialised in the reference
        best = [0.0] * (maxclique + 1)
        schnitt = self.G @ self.G[a]
        gr1 = self.G @ self.LC[a // 5]                             # |G_i & LC_a|
        gr2 = self.LC @ self.G[a]                                  # |G_a & LC_i| per column
        cov = self.LC @ self.LC[a // 5]
        cands = []
        for ii in range(self.w):
            for k in range(5):
                i = ii * 5 + k
                if i != clique[0]:
                    if schnitt[i] > self.mincov // 4:
                        Z = self.significance(int(schnitt[i]), int(cov[ii]), int(gr1[i]), int(gr2[ii]), int(self.gsize[i]), int(self.gsize[a]))
                        cands.append((Z, i))
                        if Z > greedy:
                            the_best_updater(clique, best, maxclique, i, Z)
        best[0] = 100.0
        clique[maxclique] = -1
        j = maxclique - 1
        while j > 0 and (best[j] < greedy or clique[j] == clique[j - 1]):       # RR:1231; j = 0 would read Clique[-1]: stop
            clique[j] = -1
            j -= 1
        assert all(c is not None for c in clique)
        return clique, cands

    def votes(self, members, what):
        tot = np.zeros(self.T, dtype=np.int64)
        for m in members:
            tot += self.G[m] if what == "group" else self.LC[m // 5]
        return tot

    def dropoff_cutoff(self, clique, size):
        """RR:1460-1522 with c = 0: (drop_c, min_drop)"""
        v = self.votes(clique[:size], "group")
        sizes = [float((v > k).sum()) for k in range(size)]
        drop_c = max(1, 0)
        min_drop = 1000000.0
        for i in range(drop_c, size - 1):
            if min(float(self.T) - sizes[i], sizes[i]) > 0:
                drop = (sizes[i - 1] - sizes[i + 1]) / min(float(self.T) - sizes[i], sizes[i])
                if drop < min_drop:
                    min_drop = drop
                    drop_c = i
        return drop_c, min_drop

    def refine(self):
        """Group_Refinement (RR:1634-1690) over the significant variations"""
        S = len(self.significant)
        sc = self.T // 64 + 1
        out = {"significant": np.array(self.significant, dtype=np.int32), "sizes": np.zeros(S, dtype=np.int32),
               "cliques": np.full((S, MAXCLIQUE + 1), -1, dtype=np.int32), "cutoffs": np.zeros(S, dtype=np.int32),
               "drop_off": np.full(S, 1000.0), "c_groups": np.zeros((S, sc), dtype=np.uint64),
               "c_coverage": np.zeros((S, sc), dtype=np.uint64), "candidates": [], "maxcorrs": self.maxcorrs.copy(),
               "kept": self.kept, "width": self.w, "cutoff": self.cutoff}
        for s, a in enumerate(self.significant):
            clique, cands = self.cliquer(a)
            out["cliques"][s] = clique
            out["candidates"].append(cands)
            size = 0
            while clique[size] > 0:                                # RR:1650
                size += 1
            out["sizes"][s] = size
            if size > 5:
                c, drop = self.dropoff_cutoff(clique, size)
                out["cutoffs"][s] = c
                out["drop_off"][s] = drop
                j = next(jj for jj in range(100) if clique[jj] < 0)     # RR:982-989
                out["c_groups"][s] = pack((self.votes(clique[:j], "group") > c)[None, :])[0]
                out["c_coverage"][s] = pack((self.votes(clique[:j], "coverage") > c)[None, :])[0]
            else:
                out["maxcorrs"][a] = 0.0                           # RR:1686
        return out


def ranked(cands, greedy):
    """the candidates above greedy by (Z descending, index ascending)"""
    return sorted([c for c in cands if c[0] > greedy], key=lambda c: (-c[0], c[1]))


def undecided(cands, greedy, eps=1e-8):
    """A variation whose clique a rounding difference of the tail could change: among the first 30 ranked candidates, or at
    the greedy threshold, two unequal values closer than eps."""
    r = ranked(cands, greedy)[:MAXCLIQUE]
    if any(x[0] != y[0] and abs(x[0] - y[0]) < eps for x, y in zip(r, r[1:])):
        return True
    return any(abs(z - greedy) < eps for z, _ in cands)
