"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The semantics of pgr_msa_crossovers and pgr_thread (include/pgr.h, the last two sections) restated in plain Python, character by
character over `bytes` rows and with the brute-force (k, a, b) triple loop for the crossover, for tests/test_cross.py and
tests/test_gpu_cross.py.  The reference has no counterpart for either: the header is the specification and this file restates it,
with no call into the library and no code shared with repeatresolver_amd/resolution.py.  `numpy_crossovers` gives the same
integers vectorised, for the inputs too large for the plain loops; tests/test_cross.py compares the two.  Everything returned is
an integer."""
import numpy as np

SYMBOL = {"a": 0, "A": 0, "c": 1, "C": 1, "g": 2, "G": 2, "t": 3, "T": 3, "-": 4, "_": 4}      # every other byte: 5, compared nowhere
PER_ROW = ("compared", "best", "second", "best_mismatches", "second_mismatches", "cross_split", "cross_left", "cross_right",
           "cross_mismatches", "cross_left_compared")
FIELDS = PER_ROW + ("seg_compared", "seg_best")


def first_smallest(values, without=None):
    found = -1
    for p in range(len(values)):
        if p != without and (found == -1 or values[p] < values[found]):
            found = p
    return found


def crossovers(msa, codes, von, columns, seg_end, min_side):
    """msa: bytes rows; codes[parts][width of the window] 0 .. 4; columns absolute; seg_end[nseg] ends of the segments as indices
    into columns.  A dict of numpy int32 arrays named as the fields of pgr_crossovers."""
    T, P, S = len(msa), len(codes), len(seg_end)
    out = {name: np.zeros(T, np.int32) for name in PER_ROW}
    out.update(seg_compared=np.zeros((T, S), np.int32), seg_best=np.zeros((T, S), np.int32), seg_mismatches=np.zeros((T, S, P), np.int32))
    for r in range(T):
        seg_cmp, seg_mm = [0] * S, [[0] * P for _ in range(S)]
        for s in range(S):
            for j in range(seg_end[s - 1] if s > 0 else 0, seg_end[s]):
                c = columns[j]
                x = SYMBOL.get(chr(msa[r][c]), 5)
                if x <= 4:                                             # a blank is compared nowhere; a gap is a symbol
                    seg_cmp[s] += 1
                    for p in range(P):
                        if x != int(codes[p][c - von]):
                            seg_mm[s][p] += 1
        # the one-copy explanation: pgr_msa_assign over all columns
        compared, mism = sum(seg_cmp), [sum(seg_mm[s][p] for s in range(S)) for p in range(P)]
        best = second = -1
        if compared > 0:
            best = first_smallest(mism)
            second = first_smallest(mism, without=best)
        out["compared"][r], out["best"][r], out["second"][r] = compared, best, second
        out["best_mismatches"][r] = mism[best] if best >= 0 else 0
        out["second_mismatches"][r] = mism[second] if second >= 0 else 0
        for s in range(S):
            out["seg_compared"][r, s] = seg_cmp[s]
            out["seg_best"][r, s] = first_smallest(seg_mm[s]) if seg_cmp[s] > 0 else -1
            out["seg_mismatches"][r, s] = seg_mm[s]
        # the two-copy explanation: the smallest (total, k, a, b) over the admissible splits and all pairs of different parts
        found = None
        for k in range(1, S):
            left = sum(seg_cmp[:k])
            if left < min_side or compared - left < min_side:
                continue
            for a in range(P):
                for b in range(P):
                    if a == b:
                        continue
                    total = sum(seg_mm[s][a] for s in range(k)) + sum(seg_mm[s][b] for s in range(k, S))
                    if found is None or (total, k, a, b) < found[:4]:
                        found = (total, k, a, b, left)
        total, k, a, b, left = found if found is not None else (0, -1, -1, -1, 0)
        out["cross_split"][r], out["cross_left"][r], out["cross_right"][r] = k, a, b
        out["cross_mismatches"][r], out["cross_left_compared"][r] = total, left
    return out


def numpy_crossovers(text, codes, von, columns, seg_end, min_side, rows=None):
    """the same dict from vectorised numpy, for text[T, W] uint8 and the rows `rows` of it (None: all).  The crossover goes by
    the definition too, all (k, a, b) at once per split, not by the kernel's shortcut."""
    lut = np.full(256, 5, dtype=np.uint8)
    for ch, k in SYMBOL.items():
        lut[ord(ch)] = k
    columns = np.asarray(columns, dtype=np.int64)
    sub = text if rows is None else text[np.asarray(rows)]
    pc_all = np.asarray(codes, dtype=np.uint8)
    T, P, S = sub.shape[0], pc_all.shape[0], len(seg_end)
    seg_mm, seg_cmp = np.zeros((T, S, P), np.int64), np.zeros((T, S), np.int64)
    for s in range(S):
        cols = columns[(seg_end[s - 1] if s > 0 else 0):seg_end[s]]
        rc, pc = lut[sub[:, cols]], pc_all[:, cols - von]
        matches = np.zeros((T, P), dtype=np.float32)
        for k in range(5):                                             # (exact in float32: integers far below 2^24)
            matches += (rc == k).astype(np.float32) @ (pc == k).astype(np.float32).T
        seg_cmp[:, s] = (rc <= 4).sum(axis=1)
        seg_mm[:, s] = seg_cmp[:, s, None] - matches.astype(np.int64)
    big = np.iinfo(np.int64).max
    at = np.arange(T)

    def first_two(m):                                                  # per row of m[T, P]: the first smallest and the first smallest of the others
        b = m.argmin(axis=1)
        if m.shape[1] < 2:
            return b, np.full(len(m), -1)
        o = m.copy()
        o[at, b] = big
        return b, o.argmin(axis=1)

    compared, mism = seg_cmp.sum(axis=1), seg_mm.sum(axis=1)
    best, second = first_two(mism)
    none = compared == 0
    out = {"compared": compared, "best": np.where(none, -1, best), "second": np.where(none, -1, second),
           "best_mismatches": np.where(none, 0, mism[at, best]),
           "second_mismatches": np.where(none | (second < 0), 0, mism[at, np.maximum(second, 0)]),
           "seg_compared": seg_cmp, "seg_mismatches": seg_mm,
           "seg_best": np.where(seg_cmp == 0, -1, seg_mm.argmin(axis=2))}
    split, left, right = np.full(T, -1), np.full(T, -1), np.full(T, -1)
    total, left_cmp = np.zeros(T, np.int64), np.zeros(T, np.int64)
    pre = np.cumsum(seg_mm, axis=1)
    if P >= 2:
        for k in range(1, S):
            lc = seg_cmp[:, :k].sum(axis=1)
            ok = (lc >= min_side) & (compared - lc >= min_side)
            pair = pre[:, k - 1, :, None] + (pre[:, S - 1] - pre[:, k - 1])[:, None, :]     # [T, a, b]
            pair[:, np.arange(P), np.arange(P)] = big
            flat = pair.reshape(T, P * P)
            i = flat.argmin(axis=1)                                    # the first smallest in (a, b) order
            t = flat[at, i]
            take = ok & ((split < 0) | (t < total))
            split[take], left[take], right[take], total[take], left_cmp[take] = k, (i // P)[take], (i % P)[take], t[take], lc[take]
    out.update(cross_split=split, cross_left=left, cross_right=right, cross_mismatches=total, cross_left_compared=left_cmp)
    return {name: np.asarray(v, dtype=np.int32) for name, v in out.items()}


def same(got, exp, rows=None, matrix=True):
    """a resolution.Crossovers against the dict of this file (exp covers the rows `rows` of the MSA; None: all), exactly"""
    pick = slice(None) if rows is None else np.asarray(rows)
    for name in FIELDS:
        assert np.array_equal(getattr(got, name)[pick], exp[name]), name
    if matrix:
        assert got.seg_mismatches is not None and np.array_equal(got.seg_mismatches[pick], exp["seg_mismatches"])


def thread(label_vectors):
    """pgr_thread: a dict named as the fields of pgr_threads; thread_of as a list of one list per labelling"""
    N, T = len(label_vectors), len(label_vectors[0])
    K = [max(lab) + 1 for lab in label_vectors]
    occurs = [[any(x == l for x in lab) for l in range(k)] for lab, k in zip(label_vectors, K)]
    nxt = [[-1] * k for k in K]
    has_prev = [[False] * k for k in K]
    for i in range(N - 1):
        C = [[0] * K[i + 1] for _ in range(K[i])]
        for r in range(T):
            a, b = label_vectors[i][r], label_vectors[i + 1][r]
            if a >= 0 and b >= 0:
                C[a][b] += 1
        for a in range(K[i]):
            for b in range(K[i + 1]):
                if C[a][b] <= 0:
                    continue
                row_first = all(C[a][x] < C[a][b] for x in range(b)) and all(C[a][x] <= C[a][b] for x in range(b + 1, K[i + 1]))
                col_first = all(C[x][b] < C[a][b] for x in range(a)) and all(C[x][b] <= C[a][b] for x in range(a + 1, K[i]))
                if row_first and col_first:
                    nxt[i][a] = b
                    has_prev[i + 1][b] = True
    thread_of = [[-1] * k for k in K]
    first, last = [], []
    for i in range(N):
        for a in range(K[i]):
            if occurs[i][a] and not has_prev[i][a]:
                j, l = i, a
                while True:
                    thread_of[j][l] = len(first)
                    if nxt[j][l] < 0:
                        break
                    j, l = j + 1, nxt[j][l]
                first.append(i)
                last.append(j)
    row_thread, row_conflict = [], []
    for r in range(T):
        seen = {thread_of[i][label_vectors[i][r]] for i in range(N) if label_vectors[i][r] >= 0}
        row_thread.append(seen.pop() if len(seen) == 1 else -1)
        row_conflict.append(len(seen) > 1 if row_thread[-1] < 0 else False)
    return {"nthreads": len(first), "first": first, "last": last, "thread_of": thread_of, "row_thread": row_thread,
            "row_conflict": row_conflict}


def same_threads(got, exp):
    """a resolution.Threads against the dict of `thread`, exactly"""
    assert got.nthreads == exp["nthreads"] and got.first.tolist() == exp["first"] and got.last.tolist() == exp["last"]
    assert got.nres == len(exp["thread_of"]) and got.offset.tolist() == np.cumsum([0] + [len(t) for t in exp["thread_of"]]).tolist()
    assert got.thread_of.tolist() == [x for t in exp["thread_of"] for x in t]
    assert got.row_thread.tolist() == exp["row_thread"] and got.row_conflict.tolist() == exp["row_conflict"]


def thread_labels(exp, nres, complete_only=True):
    """Threads.labels on the dict of `thread`"""
    return np.array([t if t >= 0 and (not complete_only or (exp["first"][t] == 0 and exp["last"][t] == nres - 1)) else -1
                     for t in exp["row_thread"]], dtype=np.int32)
