"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The semantics of pgr_msa_assign (include/pgr.h, last section: every row of the MSA against the consensus of every part) restated
in plain Python, character by character over `bytes` rows, for tests/test_assign.py and tests/test_gpu_assign.py.  The reference
has no counterpart for this operation: the header is the specification and this file restates it, with no call into the library
and no code shared with repeatresolver_amd/resolution.py.  `numpy_assign` gives the same integers vectorised, for the inputs too
large for the plain loops; tests/test_assign.py compares the two.  Everything returned is an integer."""
import numpy as np

SYMBOL = {"a": 0, "A": 0, "c": 1, "C": 1, "g": 2, "G": 2, "t": 3, "T": 3, "-": 4, "_": 4}      # every other byte: 5, compared nowhere


def symbol(byte):
    return SYMBOL.get(chr(byte), 5)


def compared_columns(depth, von, bis, selected=None, min_depth=1):
    """the columns resolution.assign compares: `selected` (None: every column of [von, bis]) without those at which some part
    has a depth below min_depth"""
    columns = list(range(von, bis + 1)) if selected is None else [int(x) for x in selected]
    return [x for x in columns if all(int(d[x - von]) >= min_depth for d in depth)]


def first_smallest(values, without=None):
    """the index of the smallest value, the lowest index among equals, not looking at index `without`; -1 if there is none"""
    found = -1
    for p in range(len(values)):
        if p != without and (found == -1 or values[p] < values[found]):
            found = p
    return found


def assign(msa, codes, von, columns):
    """msa: bytes rows; codes[parts][width of the window] 0 .. 4; columns absolute.  A dict of numpy int32 arrays named as the
    fields of pgr_assignment."""
    T, P = len(msa), len(codes)
    out = {"compared": np.zeros(T, np.int32), "best": np.zeros(T, np.int32), "second": np.zeros(T, np.int32),
           "best_mismatches": np.zeros(T, np.int32), "second_mismatches": np.zeros(T, np.int32), "mismatches": np.zeros((T, P), np.int32)}
    for r in range(T):
        compared, mismatches = 0, [0] * P
        for c in columns:
            s = symbol(msa[r][c])
            if s <= 4:                                                 # a blank is compared nowhere; a gap is a symbol
                compared += 1
                for p in range(P):
                    if s != int(codes[p][c - von]):
                        mismatches[p] += 1
        best = second = -1
        if compared > 0:
            best = first_smallest(mismatches)
            second = first_smallest(mismatches, without=best)
        out["compared"][r], out["best"][r], out["second"][r] = compared, best, second
        out["best_mismatches"][r] = mismatches[best] if best >= 0 else 0
        out["second_mismatches"][r] = mismatches[second] if second >= 0 else 0
        out["mismatches"][r] = mismatches
    return out


def labels(exp, part_label, min_compared, min_margin, keep=None):
    """Assignment.labels, row by row, on the dict `assign` returns"""
    out = []
    for r in range(len(exp["best"])):
        if keep is not None and keep[r] >= 0:
            out.append(int(keep[r]))
            continue
        ok = exp["best"][r] >= 0 and exp["compared"][r] >= min_compared
        if ok and exp["second"][r] != -1:
            ok = exp["second_mismatches"][r] - exp["best_mismatches"][r] >= min_margin
        out.append(int(part_label[exp["best"][r]]) if ok else -1)
    return np.array(out, dtype=np.int32)


def numpy_assign(text, codes, von, columns, rows=None):
    """the same dict from vectorised numpy, for text[T, W] uint8 and the rows `rows` of it (None: all).  A mismatch is a compared
    column without a match, and the matches are one product of one-hot matrices (exact in float32: integers far below 2^24)."""
    lut = np.full(256, 5, dtype=np.uint8)
    for ch, k in SYMBOL.items():
        lut[ord(ch)] = k
    columns = np.asarray(columns, dtype=np.int64)
    sub = text if rows is None else text[np.asarray(rows)]
    rc = lut[sub[:, columns]]                                          # [R, C]
    pc = np.asarray(codes, dtype=np.uint8)[:, columns - von]           # [P, C]
    compared = (rc <= 4).sum(axis=1).astype(np.int32)
    matches = np.zeros((rc.shape[0], pc.shape[0]), dtype=np.float32)
    for k in range(5):
        matches += (rc == k).astype(np.float32) @ (pc == k).astype(np.float32).T
    mism = compared[:, None] - matches.astype(np.int32)
    P = pc.shape[0]
    best = mism.argmin(axis=1).astype(np.int32)                        # (the first smallest)
    bm = mism[np.arange(len(mism)), best]
    if P > 1:
        other = mism.astype(np.int64)
        other[np.arange(len(mism)), best] = np.iinfo(np.int64).max
        second = other.argmin(axis=1).astype(np.int32)
        sm = mism[np.arange(len(mism)), second]
    else:
        second, sm = np.full(len(mism), -1, np.int32), np.zeros(len(mism), np.int32)
    none = compared == 0
    return {"compared": compared, "best": np.where(none, -1, best).astype(np.int32), "second": np.where(none, -1, second).astype(np.int32),
            "best_mismatches": np.where(none, 0, bm).astype(np.int32), "second_mismatches": np.where(none, 0, sm).astype(np.int32),
            "mismatches": mism.astype(np.int32)}
