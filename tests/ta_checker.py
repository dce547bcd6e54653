"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

A plain Python 3 restatement of the consensus side of the reference's TransposonAssessment.py ("TA:"): GroupMaker
(TA:159-160), Konsensus (TA:82-92), the reduction of MaxCorrs onto columns (TA:263), SignaturesMaker (TA:156-157), Diff
(TA:94-95), Resolvability (TA:97-119) and its own ResolutionQuality (TA:162-255), for tests/test_consensus.py and
tests/test_gpu_consensus.py.  It is written from the semantics, one small function per function of the script, not a copy of
its text, and it is a same-hand restatement as tests/cn_checker.py is: the script is Python 2 and no Python 2 interpreter was
available, so nothing here is pinned to an execution of the reference.  Everything it returns is an integer.

Departures, all on the surface: windows are [von, bis] with both ends inclusive, as everywhere in include/pgr.h (the script's
range(start / 5, ende / 5) is von = start // 5, bis = ende // 5 - 1: `window_of`); the consensus is returned as codes 0 .. 4
and not as characters; Diff runs on the whole consensus and a list of columns instead of on strings cut to those columns;
Resolvability returns unique[] and both lists instead of printing one and returning the other."""
import numpy as np

INDEX = {"a": 0, "c": 1, "g": 2, "t": 3, "-": 4, "A": 0, "C": 1, "G": 2, "T": 3, "_": 4}      # TA:81; anything else is 5: blank


def code(ch):
    return INDEX.get(chr(ch) if isinstance(ch, int) else ch, 5)


def load_labels(lines):
    """ResolutionLoader (TA:69-79) on the lines of a label file: an empty line is None"""
    return [None if line in ("", "\n") else int(line) for line in lines]


def groups(labels):
    """GroupMaker (TA:159-160): (the labels x in 0 .. max that occur, the rows of each); None and -1 are in no group"""
    labels = [-1 if x is None else int(x) for x in labels]
    found, members = [], []
    for x in range(max(labels) + 1):
        rows = [z for z in range(len(labels)) if labels[z] == x]
        if len(rows) > 0:
            found.append(x)
            members.append(rows)
    return found, members


def column_counts(msa, rows, column):
    """the counter of Konsensus for one column (TA:87-90): five counts, the blanks dropped"""
    counter = [0, 0, 0, 0, 0, 0]
    for z in rows:
        counter[code(msa[z][column])] += 1
    return counter[:5]


def first_maximum(counter):
    """np.argmax (TA:91): the first index of the largest value"""
    best = 0
    for k in range(1, len(counter)):
        if counter[k] > counter[best]:
            best = k
    return best


def selected_columns(maxcorrs, von, bis, cutoff):
    """TA:263 and the condition of TA:157: the columns x of [von, bis] with max(maxcorrs[5x .. 5x + 4]) > cutoff; no maxcorrs:
    all of them"""
    if maxcorrs is None:
        return list(range(von, bis + 1))
    return [x for x in range(von, bis + 1) if max(float(maxcorrs[5 * x + i]) for i in range(5)) > cutoff]


def window_of(start, ende):
    """range(start / 5, ende / 5) of TA:157 in Python 2 as an inclusive window"""
    return start // 5, ende // 5 - 1


def diff(kon1, kon2, columns):
    """Diff (TA:94-95) on two consensus given as codes, over `columns` (indices into them): a consensus is never blank"""
    return len([1 for t in columns if kon1[t] != kon2[t]])


def consensus(msa, labels, von=None, bis=None, maxcorrs=None, cutoff=1.0):
    """everything pgr_msa_consensus returns, as a dict of numpy arrays"""
    width = len(msa[0])
    if von is None and bis is None:
        von, bis = 0, width - 1
    W = bis + 1 - von
    found, members = groups(labels)
    P = len(found)
    counts = np.zeros((P, W, 5), dtype=np.int32)
    kon = np.zeros((P, W), dtype=np.uint8)
    for p in range(P):
        for c in range(W):
            counter = column_counts(msa, members[p], von + c)
            counts[p, c] = counter
            kon[p, c] = first_maximum(counter)
    selected = selected_columns(maxcorrs, von, bis, cutoff)
    inside = [x - von for x in selected]
    d = np.zeros((P, P), dtype=np.int32)
    d_all = np.zeros((P, P), dtype=np.int32)
    kons = kon.tolist()                                                # (plain lists: the same comparisons, faster than numpy scalars)
    for p in range(P):
        for q in range(P):
            d[p, q] = diff(kons[p], kons[q], inside)
            d_all[p, q] = diff(kons[p], kons[q], range(W))
    return {"von": von, "bis": bis, "part_label": np.array(found, dtype=np.int32),
            "part_rows": np.array([len(m) for m in members], dtype=np.int32), "counts": counts, "depth": counts.sum(axis=2),
            "consensus": kon, "selected": np.array(selected, dtype=np.int32), "diff": d, "diff_all": d_all}


def tied_columns(counts):
    """the (part, column) pairs whose largest count is reached twice and is not 0: where the first-maximum rule decides"""
    top = counts.max(axis=2)
    return int((((counts == top[:, :, None]).sum(axis=2) > 1) & (top > 0)).sum())


def resolvability(diffs):
    """Resolvability (TA:97-119) on the matrix of Diff values: (summe[11], the smallest diff of every part, MinDiffs as the
    script returns it).  TA:112 appends `diff` -- the value of the last kk != k --, not `mindiff`."""
    n = len(diffs)
    if n < 2:
        raise NameError("diff")                                        # TA:112 reads a name no iteration has set
    summe = [0] * 11
    smallest, returned = [], []
    for k in range(n):
        unique = [1] * 11
        mindiff = 1000000
        last = None
        for kk in range(n):
            if k != kk:
                last = int(diffs[k][kk])
                if last < mindiff:
                    mindiff = last
                for t in range(last, len(unique)):
                    unique[t] = 0
        returned.append(last)
        smallest.append(mindiff)
        for t in range(len(unique)):
            summe[t] += unique[t]
    return summe, smallest, returned


def resolution_quality(truth, labels):
    """ResolutionQuality (TA:162-255): (truepositives, falsepositives, conconfpositives).  A truth group's size counts all its
    rows (TA:178), also those whose label is -1."""
    truth = [-1 if x is None else int(x) for x in truth]
    labels = [-1 if x is None else int(x) for x in labels]
    _, members = groups(truth)
    G, K = len(members), max(labels) + 1
    m1 = np.zeros((G, K))
    m2 = np.zeros((K, G))
    for g in range(G):                                                 # TA:177-180
        size = float(len(members[g]))
        for k in range(K):
            m1[g][k] = float(len([z for z in members[g] if labels[z] == k])) / size
    for k in range(K):                                                 # TA:182-186
        size = float(labels.count(k))
        for g in range(G):
            if size > 0:
                m2[k][g] = float(len([z for z in members[g] if labels[z] == k])) / size
    m3 = np.dot(m1, m2)                                                # TA:188
    for g in range(G):                                                 # TA:191-195
        summe = sum(m3[g][t] for t in range(G))
        for t in range(G):
            if summe > 0.0:
                m3[g][t] /= summe
    positives = [0] * 10
    true_pos = false_pos = 0
    for t in range(G):                                                 # TA:229-248
        maxi, maxtt = 0.0, 0
        for tt in range(G):
            if m3[t][tt] > maxi:
                maxi, maxtt = m3[t][tt], tt
        if maxi == max(m3[maxtt]):
            if maxtt != t:
                false_pos += 1
            else:
                true_pos += 1
                for c in range(10):
                    if maxi > float(c) / 10.0:
                        positives[c] += 1
    return true_pos, false_pos, positives
