"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The inputs tests/test_cross.py (no GPU) and tests/test_gpu_cross.py share: the
hand-made case of tests/cs_cases.py extended by a row that changes part at a boundary, with its outcome worked out by hand; the
labellings on which pgr_thread is pinned; the noise-free splices and the ties.  Everything compared is an integer: every
comparison is exact."""
import numpy as np

import as_cases as asc
import cs_cases as cs

MAX_SEGMENTS = 1024                                                   # PGR_CX_MAX_SEGMENTS of include/pgr.h

# cs_cases.HAND_ROWS and one more row, in no part, against cs_cases.HAND_CONSENSUS over as_cases.HAND_COLUMNS = 0 1 3 4 5 6 7 8 in
# two segments, seg_end = 3 8: columns 0 1 3 | columns 4 5 6 7 8, where
#   part 0 is  a g a | - t c g t
#   part 1 is  c g c | - t g - t
# row 6  a g a | - t g - t  is part 0 left of the boundary and part 1 right of it (column 2, an 'a', is not compared).
#          segment 0 (part 0, part 1)      segment 1 (part 0, part 1)         one copy          (0,1)  (1,0)  crossover
# row 0  a g A: 0, 2 (columns 0 3)       _ t c g T: 0, 2 (columns 6 7)       0 4: 0 then 1      2      2      k 1, 0 -> 1, 2
# row 1  c - a: 2 (0 1), 2 (1 3)         - t C - .: 4 compared; 1 (7), 1 (6) 3 3: tie, 0 then 1 3      3      k 1, 0 -> 1, 3
# row 2  c g a: 1 (0), 1 (3)             - t g g t: 1 (6), 1 (7)             2 2: tie           2      2      k 1, 0 -> 1, 2
# row 3  C g c: 2 (0 3), 0               _ t g - t: 2 (6 7), 0               4 0: 1 then 0      2      2      k 1, 0 -> 1, 2
# row 4  t t t: 3, 3                     t t t t t: 3 (4 6 7), 3 (4 6 7)     6 6: tie           6      6      k 1, 0 -> 1, 6
# row 5  c - c: 3, 1 (1)                 a . a - .: 3 compared; 3, 2 (4 6)   6 3: 1 then 0      5      4      k 1, 1 -> 0, 4
# row 6  a g a: 0, 2 (0 3)               - t g - t: 2 (6 7), 0               2 2: tie           0      4      k 1, 0 -> 1, 0
# Every row has three compared columns left of the boundary.  A tie between (0, 1) and (1, 0) goes to the lower a.  Only row 6
# gains by the crossover: 2 - 0 = 2; rows 0 and 3 lose 2, row 5 loses 1, the ties gain nothing.
HAND_ROWS = cs.HAND_ROWS + [b"agaa-tg-t"]
HAND_COLUMNS = asc.HAND_COLUMNS
HAND_SEG_END = [3, 8]
HAND_SEG_COMPARED = [[3, 5], [3, 4], [3, 5], [3, 5], [3, 5], [3, 3], [3, 5]]
HAND_SEG_MISMATCHES = [[[0, 2], [0, 2]], [[2, 2], [1, 1]], [[1, 1], [1, 1]], [[2, 0], [2, 0]], [[3, 3], [3, 3]], [[3, 1], [3, 2]],
                       [[0, 2], [2, 0]]]
HAND_SEG_BEST = [[0, 0], [0, 0], [0, 0], [1, 1], [0, 0], [1, 1], [0, 1]]
HAND_COMPARED = asc.HAND_COMPARED + [8]
HAND_BEST = asc.HAND_BEST + [0]
HAND_SECOND = asc.HAND_SECOND + [1]
HAND_BEST_MISMATCHES = [0, 3, 2, 0, 6, 3, 2]
HAND_SECOND_MISMATCHES = [4, 3, 2, 4, 6, 6, 2]
HAND_CROSS_SPLIT = [1] * 7
HAND_CROSS_LEFT = [0, 0, 0, 0, 0, 1, 0]
HAND_CROSS_RIGHT = [1, 1, 1, 1, 1, 0, 1]
HAND_CROSS_MISMATCHES = [2, 3, 2, 2, 6, 4, 0]
HAND_CROSS_LEFT_COMPARED = [3] * 7
HAND_ROWS_GAIN_1 = [6]
# min_side 4: no row has four compared columns left of the boundary, so no split is admissible: -1 -1 -1 0 0 everywhere


def hand_expected():
    return {"compared": HAND_COMPARED, "best": HAND_BEST, "second": HAND_SECOND, "best_mismatches": HAND_BEST_MISMATCHES,
            "second_mismatches": HAND_SECOND_MISMATCHES, "seg_compared": HAND_SEG_COMPARED, "seg_best": HAND_SEG_BEST,
            "seg_mismatches": HAND_SEG_MISMATCHES, "cross_split": HAND_CROSS_SPLIT, "cross_left": HAND_CROSS_LEFT,
            "cross_right": HAND_CROSS_RIGHT, "cross_mismatches": HAND_CROSS_MISMATCHES, "cross_left_compared": HAND_CROSS_LEFT_COMPARED}


def equal_segments(n, segments):
    """`segments` segments of as equal a number of the n compared columns as possible: what resolution.crossovers makes of `segments`"""
    return [(s + 1) * n // segments for s in range(segments)]


LETTERS = np.frombuffer(b"acgt-", dtype=np.uint8)


def splices(seed, parts, ncolumns, seg_end, rows, spliced):
    """Noise-free rows: (text [rows, ncolumns] uint8, codes, what[rows]): codes are random but no two parts agree in any segment;
    row r is part r mod parts written as letters, but for `spliced` of the rows, which are part A left of a segment boundary and
    part B != A right of it: what[r] = (k, A, B), or None for an unspliced row."""
    rng = np.random.default_rng(seed)
    codes = asc.random_codes(seed, parts, ncolumns).copy()
    lo = 0
    for e in seg_end:                                                  # part p alone has code (p + x) % 5 at p's own column of every segment
        assert e - lo >= parts
        for p in range(parts):
            codes[:, lo + p] = (np.arange(parts) == p) * 1 + rng.integers(0, 4)
        lo = e
    text, what = LETTERS[codes[np.arange(rows) % parts]], [None] * rows
    for r in rng.choice(rows, size=spliced, replace=False):
        a = r % parts
        b = int((a + 1 + rng.integers(0, parts - 1)) % parts)
        k = int(rng.integers(1, len(seg_end)))
        text[r, seg_end[k - 1]:] = LETTERS[codes[b, seg_end[k - 1]:]]
        what[r] = (k, a, b)
    return text, codes, what


# ---- pgr_thread: the labellings of tests/test_cross.py, also run by the stand-alone sanitizer program (same numbers there) ----
THREAD_CASES = {
    # three identical labellings of three parts: three threads, each spanning everything
    "identical": [[0, 0, 1, 1, 2, 2, -1]] * 3,
    # part 0 splits into 0 and 1 (3 rows and 2): the larger half continues the thread, the smaller starts one
    "split": [[0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 2, 2, 2]],
    # part 1 vanishes in the middle labelling (its rows are -1 there) and reappears: two threads for it
    "vanish": [[0, 0, 0, 1, 1, 1], [0, 0, 0, -1, -1, -1], [0, 0, 0, 1, 1, 1]],
    # ties: label 0 shares two rows with each of 0 and 1 (the first largest of its row is 0); labels 0 and 1 of the first
    # labelling share two rows each with label 2 of the second (the first largest of that column is 0)
    "ties": [[0, 0, 0, 0, 0, 0, 1, 1, 2], [0, 0, 1, 1, 2, 2, 2, 2, 3]],
    # rows at -1 in some labelling, in all, and a label value that no row holds (2 in the first labelling)
    "minus": [[0, -1, 0, 1, -1, 3, 3], [0, 0, -1, 1, -1, 2, 2], [-1, 0, 0, 1, -1, 2, -1]],
    # row 6 is labelled 0 in the first labelling and 1 in the second, on two different threads: a conflict
    "conflict": [[0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, 1]],
}


def random_labellings(seed=3, rows=300, nres=5, parts=6):
    """5 labellings of 300 rows: a truth of 6 copies, in every labelling a tenth of the rows left out, a tenth relabelled at
    random and the labels permuted"""
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, parts, size=rows)
    out = []
    for _ in range(nres):
        lab = rng.permutation(parts + 1)[truth]
        noise = rng.random(rows)
        lab = np.where(noise < 0.1, -1, np.where(noise < 0.2, rng.integers(0, parts + 1, size=rows), lab))
        out.append(lab.astype(np.int32).tolist())
    return out
