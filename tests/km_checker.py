"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

A literal restatement, in plain Python and numpy, of the last subdivision stage of the reference's RepeatResolver.c ("RR:"):
Kmeans_Subdivision (RR:3382-3403) with Relative_Vars (RR:2424-2493), Relative_Group_Significance and CumHypGeo_Log
(RR:490-522) and Kmeans (RR:2604-2821), on a gr_checker.Window and the kept-row labels sd_checker leaves after
RelativeDropoff_Subdivision.  None of the product's shortcuts is used: the k loop stays, Relative_Vars is run anew for
every part, the top-5 list is sorted swap for swap before every j, the reassignment is the sequential chain.

The only floating point is mco_hyper_P / mco_hyper_Q of oracle/libmcoracle.so (the tails the reference binary of the
fixtures was linked with, through oracle/gsl_standin.c) followed by one log10.  Counts are exact integer sums over 0/1 rows;
GrMatch (RR:163-175) with the temporary sc = varzahl / 64 + 1 of RR:2625 is sc * 64 minus the number of differing bits.

PINNED to the reference: tests/test_kmeans_subdivision.py compares subdivision_bytes of the labels with the
KmeansSubdivisionOf_ files in tests/golden/rr_kmeans_reference.json.gz (scripts/gen_km_fixtures.py)."""
import ctypes
import functools
import math

import numpy as np

import gr_checker as gc
import sd_checker as sd

MIN_DISTANCE = 100                                                  # RR:2462: j starts at i + 100


@functools.lru_cache(maxsize=None)
def _tails():
    lib = gc.mco()
    lib.mco_hyper_P.restype = ctypes.c_double
    lib.mco_hyper_P.argtypes = [ctypes.c_uint] * 4
    return lib


@functools.lru_cache(maxsize=None)
def cum_hyp_geo_log(schnitt, gr1, gr2, cov):
    """RR:490-504; the arguments are unsigned there: schnitt - 1 wraps at 0, and Q of 4294967295 is 0"""
    lib = _tails()
    posP = lib.mco_hyper_P(schnitt, gr2, cov - gr2, gr1)
    posQ = lib.mco_hyper_Q((schnitt - 1) & 0xFFFFFFFF, gr2, cov - gr2, gr1)
    pos = posP if (posP < posQ or schnitt == 0) else posQ           # RR:495
    if pos < 0.0:
        return math.nan                                                # log10 of a negative 1 - sum: NaN there, and `Z > cutoff` is false
    z = -1.0 * math.log10(pos) if pos > 0.0 else math.inf
    if math.isinf(z) or z > 99:
        return 99.0
    return z


def relative_group_significance(g1, g2, cov):
    """RR:506-522 on 0/1 rows"""
    schnitt = int((g1 & g2 & cov).sum())
    c = int(cov.sum())
    gr1 = int((g1 & cov).sum())
    gr2 = int((g2 & cov).sum())
    if gr1 == 0 or gr2 == 0:
        return 0.0
    z = cum_hyp_geo_log(schnitt, gr1, gr2, c)
    if math.isinf(z) or z > 99.0:
        z = 99.0
    return z


def relative_vars(win, U, u_no, maxcorrs, cutoff, mingroup):
    """RR:2424-2493.  Returns (Vars ascending, [(i, j, Z)] of every evaluated pair, in the order of evaluation)."""
    V = win.V
    selected = [1 if maxcorrs[i] > cutoff else 0 for i in range(V)]    # RR:2430-2434
    u_group = (U == u_no).astype(np.int64)                             # RR:2438
    for i in range(V):                                                 # RR:2444-2450
        if selected[i]:
            if int((u_group & win.G[i]).sum()) < mingroup:
                selected[i] = 0
    pairs = []
    # RR:2458-2476.  SelectedVars only ever goes from 1 to 2 in here and both pass `if(SelectedVars[j])`, so the variations
    # the two loops stop at are the ones marked now; walking that list instead of every index changes nothing.
    marked = [i for i in range(V) if selected[i]]
    for i in marked:
        for j in marked:
            if j < i + MIN_DISTANCE:
                continue
            Z = relative_group_significance(win.G[j], win.G[i], u_group)
            pairs.append((i, j, Z))
            if Z > cutoff:
                selected[i] = 2
                selected[j] = 2
    return [i for i in range(V) if selected[i] == 2], pairs


def exchange_sort_5(best_score, best_j):
    """RR:2667-2681, swap for swap, in place"""
    for k in range(5):
        for l in range(k + 1, 5):
            if best_score[l] < best_score[k]:
                best_score[l], best_score[k] = best_score[k], best_score[l]
                best_j[l], best_j[k] = best_j[k], best_j[l]


def top5(scores):
    """RR:2658-2688 for one row i: scores[j] = GrMatch(VarSigs[j], VarSigs[i]) for j ascending.  Returns best_j[5]."""
    best_score = [0] * 5
    best_j = [0] * 5
    for j in range(len(scores)):
        score = scores[j]
        exchange_sort_5(best_score, best_j)
        if score > best_score[0]:
            best_score[0] = score
            best_j[0] = j
    return best_j


def match_matrix(A, B, sc_km):
    """GrMatch(A[j], B[i]) for all (i, j) at once: [len(B), len(A)] exact integers (bits beyond varzahl are 0 in both)"""
    A = A.astype(np.int64)
    B = B.astype(np.int64)
    differing = B.sum(axis=1)[:, None] + A.sum(axis=1)[None, :] - 2 * (B @ A.T)
    return sc_km * 64 - differing


def reassign(scores, clusternumber, mingroup):
    """RR:2726-2755 on scores[i][j] = GrMatch(Centroids[j], VarSigs[i]); clusternumber in place.  Returns the moves
    [(min, i, from, to)]."""
    anzahl = len(clusternumber)
    clustersize = [0] * anzahl
    for i in range(anzahl):
        clustersize[clusternumber[i]] += 1
    moves = []
    for mn in range(2, mingroup):
        for i in range(anzahl):
            if clustersize[clusternumber[i]] <= mn:
                best_score, best_j = 0, 0
                row = scores[i]
                for j in range(anzahl):
                    if clustersize[j] >= mn and clusternumber[i] != j:
                        score = row[j]
                        if score > best_score and i != j:
                            best_score = score
                            best_j = j
                moves.append((mn, i, clusternumber[i], best_j))
                clustersize[clusternumber[i]] -= 1
                clusternumber[i] = best_j
                clustersize[best_j] += 1
    return moves


def kmeans(win, U, u_no, Vars, mingroup):
    """RR:2604-2821 on U in place.  Returns a dict: rows (I), varzahl, before / after (Clusternumber before and after the
    reassignment), moves."""
    I = [i for i in range(win.T) if U[i] == u_no]                      # RR:2616-2623
    anzahl, varzahl = len(I), len(Vars)
    sc_km = varzahl // 64 + 1                                          # RR:2625
    var_sigs = np.zeros((anzahl, sc_km * 64), dtype=np.int64)          # RR:2633-2640
    for j in range(varzahl):
        var_sigs[:, j] = win.G[Vars[j]][I]
    own = match_matrix(var_sigs, var_sigs, sc_km).tolist()
    centroids = np.zeros((anzahl, sc_km * 64), dtype=np.int64)
    for i in range(anzahl):                                            # RR:2656-2703
        best_j = top5(own[i])
        s = var_sigs[best_j].sum(axis=0)                               # RR:2694-2702: the five rows, repeats counted again
        centroids[i, :varzahl] = (s > 2)[:varzahl]
    scores = match_matrix(centroids, var_sigs, sc_km).tolist()         # [i][j] = GrMatch(Centroids[j], VarSigs[i])
    clusternumber = [0] * anzahl
    for i in range(anzahl):                                            # RR:2706-2723
        best_score, best_j = 0, 0
        row = scores[i]
        for j in range(anzahl):
            if row[j] > best_score and i != j:
                best_score = row[j]
                best_j = j
        clusternumber[i] = best_j
    before = list(clusternumber)
    moves = reassign(scores, clusternumber, mingroup)
    max_u = 0
    for i in range(win.T):                                             # RR:2813-2815
        if U[i] > max_u:
            max_u = int(U[i])
    for i in range(anzahl):
        U[I[i]] = clusternumber[i] + max_u + 1
    return {"rows": I, "varzahl": varzahl, "before": before, "after": list(clusternumber), "moves": moves}


def kmeans_subdivision(win, ref, U, mingroup):
    """RR:3382-3403 on U (the kept rows' labels) in place.  Returns (parts before, parts after, [per eligible part a dict:
    part, vars, pairs, and what kmeans returns])."""
    number = sd.unterteilungskomprimierung(U)
    done = []
    for k in range(number):
        count = int((U == k).sum())
        if count > mingroup * 2:
            Vars, pairs = relative_vars(win, U, k, ref["maxcorrs"], ref["cutoff"], mingroup)
            rec = {"part": k, "vars": Vars, "pairs": pairs}
            rec.update(kmeans(win, U, k, Vars, mingroup))
            done.append(rec)
    after = sd.unterteilungskomprimierung(U)
    return number, after, done


def clustered(win, ref, reldrop_labels, cov):
    """main() RR:4064-4075 without the file: labels after UnterteilungsKomplettierung and the per-part records"""
    U = np.array(reldrop_labels, dtype=np.int64)[np.asarray(ref["kept"], dtype=bool)]
    before, after, parts = kmeans_subdivision(win, ref, U, cov // 2)
    return {"labels": sd.unterteilungskomplettierung(U, ref["kept"]), "parts_before": before, "parts": after, "eligible": parts}


def margin(parts, cutoff):
    """the smallest distance of an evaluated pair's Z from the cutoff (inf: no pair; a NaN counts as on the cutoff)"""
    return min((0.0 if math.isnan(z) else abs(z - cutoff) for p in parts for _, _, z in p["pairs"]), default=math.inf)
