"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

A literal restatement, in plain Python and numpy, of the two subdivision stages of the reference's RepeatResolver.c ("RR:")
that include/pgr.h covers, loop for loop: DropOff_Subdivision (RR:3180-3271, with its exchange sort),
RelativeDropoff_Subdivision (RR:3274-3378) with Relative_Dropoff_Cutoff (RR:2859-2920) and a fresh CliqueGroup
(RR:976-1008) for every pair (partition k, selected variation i), Unterteilungskomprimierung (RR:1823-1843),
UnterteilungsKomplettierung (RR:1845-1865) and the file writer (RR:568-585).  Unterteilung_Assessment (RR:2824-2856) only
prints and is left out.  None of the product's shortcuts is used here: the k x i double loop stays, every later i after a
split is still evaluated, and the votes are counted anew for every pair.

Inputs: a gr_checker.Window (Groups as 0/1 rows, signumber = T) and the dict gr_checker.Window.refine() returns (or one
built by hand with the same keys).  The reference's arrays are indexed by the variation; here `ref` is indexed by the entry
s with ref["significant"][s] = the variation, ascending, so "I" below holds entries and orders exactly as the reference's.
All results are integers; the only floating point is the drop, one division of exactly representable integers.

PINNED to the reference as gr_checker.py is: tests/test_rr_reference.py compares subdivision_bytes of both stages with the
label files of the unmodified RepeatResolver.c linked with a stand-in for its three GSL functions (not a GSL-linked binary)."""
import numpy as np

DROPOFFCUTOFF = 0.0001                                              # RR:4036
SIZECUTOFF = -1                                                     # RR:4027


def selected(ref):
    """RR:3186-3193 / RR:3279-3286: MaxCorrs[i] > cutoff && Sizes[i] > sizecutoff, ascending in i"""
    return [s for s in range(len(ref["significant"]))
            if ref["maxcorrs"][ref["significant"][s]] > ref["cutoff"] and ref["sizes"][s] > SIZECUTOFF]


def exchange_sort(I, drop_off, sizes, maxcorrs):
    """RR:3199-3213, swap for swap: Drop_Off ascending, then Sizes descending, then MaxCorrs descending.  Not stable."""
    I = list(I)
    anzahl = len(I)
    for i in range(anzahl):
        for j in range(i + 1, anzahl):
            if drop_off[I[i]] > drop_off[I[j]]:
                I[i], I[j] = I[j], I[i]
            elif drop_off[I[i]] == drop_off[I[j]]:
                if sizes[I[i]] < sizes[I[j]]:
                    I[i], I[j] = I[j], I[i]
                elif sizes[I[i]] == sizes[I[j]]:
                    if maxcorrs[I[i]] < maxcorrs[I[j]]:
                        I[i], I[j] = I[j], I[i]
    return I


def unterteilungskomprimierung(U):
    """RR:1823-1843: renumber by first appearance, in place; returns the number of parts"""
    mx = 0
    for i in range(len(U)):
        if mx < U[i]:
            mx = int(U[i])
    replace = [-1] * (mx + 1)
    mx = 0
    for i in range(len(U)):
        if U[i] > -1:
            if replace[U[i]] < 0:
                replace[U[i]] = mx
                mx += 1
            U[i] = replace[U[i]]
    return mx


def unterteilungskomplettierung(U, kept):
    """RR:1845-1865: one label per input row, -1 for the rows left out"""
    out, j = [], 0
    for i in range(len(kept)):
        if kept[i]:
            out.append(int(U[j]))
            j += 1
        else:
            out.append(-1)
    return np.array(out, dtype=np.int32)


def unpack(words, T):
    """uint64 [sc] -> 0/1 [T] (GrElement, RR:262-269)"""
    return np.array([(int(words[r // 64]) >> (r % 64)) & 1 for r in range(T)], dtype=np.int64)


def dropoff_subdivision(win, ref, mingroup, sort=exchange_sort):
    """RR:3180-3271.  Returns (Unterteilung[T], number, I after the sort)."""
    I = selected(ref)
    mc = [ref["maxcorrs"][v] for v in ref["significant"]]
    I = sort(I, ref["drop_off"], ref["sizes"], mc)
    T = win.T
    U = np.zeros(T, dtype=np.int64)
    number = 1
    number2 = 1
    for i in range(len(I)):
        if ref["drop_off"][I[i]] < DROPOFFCUTOFF:                   # RR:3227
            cg = unpack(ref["c_groups"][I[i]], T)
            for k in range(number):
                ink = U == k
                drinne = int((ink & (cg == 1)).sum())               # RR:3233-3242
                draus = int((ink & (cg == 0)).sum())
                if drinne > mingroup and draus > mingroup:
                    U[ink & (cg == 1)] = number2                    # RR:3246-3255
                    U[ink & (cg == 0)] = number2 + 1
                    number2 += 2
            number = number2
            number = unterteilungskomprimierung(U)
    return U, number, I


def relative_dropoff_cutoff(win, clique, size, c, U, u_no):
    """RR:2859-2920: (drop_c, min_drop) of the first `size` members' votes among the rows of partition u_no"""
    v = win.votes(clique[:size], "group") * (U == u_no)             # RR:2870-2881: ii counts only rows of u_no
    sizes = [float((v > t).sum()) for t in range(size)]             # Cutoff_Groups[t]: in more than t groups
    drop_c = max(1, c)
    min_drop = 1000000.0
    for i in range(drop_c, size - 1):
        if min(float(win.T) - sizes[i], sizes[i]) > 0:              # RR:2898: the whole signumber, not the partition's size
            drop = (sizes[i - 1] - sizes[i + 1]) / min(float(win.T) - sizes[i], sizes[i])
            if drop < min_drop:
                min_drop = drop
                drop_c = i
    return drop_c, min_drop


def clique_group(win, clique, c):
    """RR:976-1008 as 0/1 [T]: all members up to the first negative entry"""
    j = next(jj for jj in range(100) if clique[jj] < 0)
    return (win.votes(clique[:j], "group") > c).astype(np.int64)


def relativedropoff_subdivision(win, ref, U, mingroup):
    """RR:3274-3378 on U in place.  Returns (number before, number after, splits): splits = [(k, entry, c)] in the order they
    happen.  Drop_Off is overwritten as in the reference (RR:2912), on a copy; best_dropoff / bestgroup_i (RR:3313-3333) are
    computed from it in the reference and never used, so they are not restated."""
    I = selected(ref)
    drop_off = np.array(ref["drop_off"], dtype=np.float64)
    number = unterteilungskomprimierung(U)                          # RR:3288
    splits = []
    for k in range(number):
        count = int((U == k).sum())
        if count > mingroup * 2:                                    # RR:3303
            for i in range(len(I)):
                s = I[i]
                clique = [int(x) for x in ref["cliques"][s]]
                c, drop_off[s] = relative_dropoff_cutoff(win, clique, int(ref["sizes"][s]), 0, U, k)
                cg = clique_group(win, clique, c)                   # RR:3312
                if drop_off[s] < DROPOFFCUTOFF:                     # RR:3336
                    ink = U == k
                    drinne = int((ink & (cg == 1)).sum())
                    draus = int((ink & (cg == 0)).sum())
                    if drinne > mingroup and draus > mingroup:
                        U[ink & (cg == 1)] = number + 1 + k * 2     # RR:3359-3360
                        U[ink & (cg == 0)] = number + 2 + k * 2
                        splits.append((k, s, c))
    after = unterteilungskomprimierung(U)                           # RR:3371
    return number, after, splits


def subdivide(win, ref, cov, sort=exchange_sort):
    """main() RR:4027-4062 without the files: a dict with both label arrays (after UnterteilungsKomplettierung), the part
    counts, per stage-1 part the winning variation and its cutoff (-1: none), the splits and the sorted I"""
    mingroup = cov // 2                                             # RR:4028
    U, n1, I = dropoff_subdivision(win, ref, mingroup, sort)
    drop = unterteilungskomplettierung(U, ref["kept"])
    before, n2, splits = relativedropoff_subdivision(win, ref, U, mingroup)
    assert before == n1 or win.T == 0                               # no kept row: RR:3288 counts 0 parts, stage 1 started at 1
    rel = unterteilungskomplettierung(U, ref["kept"])
    assert len({k for k, _, _ in splits}) == len(splits), "a partition split twice: the product's shortcut 2 would not hold"
    winner = np.full(n1, -1, dtype=np.int32)
    winner_cutoff = np.full(n1, -1, dtype=np.int32)
    for k, s, c in splits:
        winner[k] = ref["significant"][s]
        winner_cutoff[k] = c
    return {"dropoff_labels": drop, "reldrop_labels": rel, "dropoff_parts": n1, "reldrop_parts": n2, "winner": winner,
            "winner_cutoff": winner_cutoff, "splits": splits, "I": I, "selected": len(selected(ref))}


def subdivision_bytes(labels):
    """RR:578-583: decimal labels separated by newlines, none at the end"""
    out = b""
    for i in range(len(labels)):
        if i != 0:
            out += b"\n"
        out += b"%d" % int(labels[i])
    return out


def subdivision_name(stage, von, bis, msa):
    """RR:3962-3965, RR:4041-4046: von / bis as main() holds them after RR:3948-3952 (Einlesen gets them by value, so its
    clipping of bis at RR:328 does not reach main): 0 and 1500000 for the whole width"""
    if von is None and bis is None:
        von, bis = 0, 1500000
    return "%sSubdivisionOf_%d_%d_%s" % (stage, von, bis, msa)
