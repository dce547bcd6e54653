"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The inputs tests/test_assign.py (no GPU) and tests/test_gpu_assign.py share: the
outcome of the hand-made 6 x 9 case of tests/cs_cases.py worked out by hand, the main input with what tests/as_checker.py gives
for it (computed once per process), the random inputs of the geometry tests and the comparison of a resolution.Assignment with
the checker's dict.  Everything compared is an integer: every comparison is exact."""
import functools

import numpy as np

import as_checker as ac
import cs_cases as cs
import ta_checker as ta

KERNEL_TILE = 8                                                       # PGR_AS_TILE of include/pgr.h: parts per work-group of k_as_dist and k_st_dist (row_planes.h)
KERNEL_SCRATCH_BYTES = 64 << 20                                       # PGR_AS_SCRATCH_BYTES: planes and matrix of one range of rows
FIELDS = ("compared", "best", "second", "best_mismatches", "second_mismatches")

# cs_cases.HAND_ROWS against HAND_CONSENSUS, window [0, 8], every column, min_depth 1.  Column 2 drops out (part 0 has depth 0
# there): the compared columns are 0 1 3 4 5 6 7 8, where
#   part 0 (label 0) is  a g a - t c g t   = 0 2 0 4 3 1 2 3
#   part 1 (label 2) is  c g c - t g - t   = 1 2 1 4 3 2 4 3
# row 0  a g A _ t c g T  all eight compared; equals part 0; differs from part 1 in columns 0 3 6 7
# row 1  c - a - t C - .  column 8 blank: 7 compared; part 0: columns 0 1 7; part 1: columns 1 3 6; a tie, the lower index is best
# row 2  c g a - t g g t  part 0: columns 0 6; part 1: columns 3 7; a tie
# row 3  C g c _ t g - t  part 0: columns 0 3 6 7; equals part 1
# row 4  t t t t t t t t  matches both only in columns 5 and 8: 6 and 6; a tie
# row 5  c - c a . a - .  columns 5 and 8 blank: 6 compared; part 0: all six; part 1: columns 1 (- / g), 4 (a / -), 6 (a / g)
HAND_COLUMNS = [0, 1, 3, 4, 5, 6, 7, 8]
HAND_COMPARED = [8, 7, 8, 8, 8, 6]
HAND_MISMATCHES = [[0, 4], [3, 3], [2, 2], [4, 0], [6, 6], [6, 3]]
HAND_BEST = [0, 0, 0, 1, 0, 1]
HAND_SECOND = [1, 1, 1, 0, 1, 0]
# the same over cs_cases.HAND_SELECTED = 0 2 3 7 8, of which column 2 drops out: 0 3 7 8, where part 0 is a a g t = 0 0 2 3 and
# part 1 is c c - t = 1 1 4 3
# row 0  a A g T: (0, 3) | row 1  c a - .: 3 compared, part 0: columns 0 7, part 1: column 3 | row 2  c a g t: (1, 2)
# row 3  C c - t: (3, 0) | row 4  t t t t: (3, 3) | row 5  c c - .: 3 compared, (3, 0)
HAND_SEL_COLUMNS = [0, 3, 7, 8]
HAND_SEL_COMPARED = [4, 3, 4, 4, 4, 3]
HAND_SEL_MISMATCHES = [[0, 3], [2, 1], [1, 2], [3, 0], [3, 3], [3, 0]]
HAND_SEL_BEST = [0, 1, 0, 1, 0, 1]
HAND_SEL_SECOND = [1, 0, 1, 0, 1, 0]


def same(got, exp, rows=None, matrix=True):
    """a resolution.Assignment against the dict of as_checker (exp covers the rows `rows` of the MSA; None: all), exactly"""
    pick = slice(None) if rows is None else np.asarray(rows)
    for name in FIELDS:
        assert np.array_equal(getattr(got, name)[pick], exp[name]), name
    if matrix:
        assert got.mismatches is not None and np.array_equal(got.mismatches[pick], exp["mismatches"])


# One hand-made row appended to ragged(31), in no part of any labelling: ragged(31) alone has no row that ties between best and
# second in its second window.  A row of gaps has a symbol in every compared column and differs from every part wherever the
# part's consensus is a base -- at every compared column of this input --, so all four parts tie.
def extra_rows(width):
    return [b"-" * width]


@functools.lru_cache(maxsize=None)
def main_input():
    """(rows, text, MaxCorrs, per window of SITES a dict): ragged(31) of tests/test_gpu_resolve.py and a row of gaps appended, the
    checker chain's k-means labels (-1 for the appended row), their consensus by ta_checker with the cutoff cs_cases.CUTOFF, the
    compared columns (selected, every part of depth >= 1) and what as_checker.assign gives"""
    from test_gpu_resolve import SITES, checker_chain
    rows, mc, chain = checker_chain()
    rows = list(rows) + extra_rows(len(rows[0]))
    text = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)
    out = []
    for (von, bis), c in zip(zip(SITES[:-1], SITES[1:]), chain):
        labels = np.concatenate([c["km"]["labels"], np.full(len(rows) - len(c["km"]["labels"]), -1)]).astype(np.int32)
        con = ta.consensus(rows, labels, von, bis, mc, cs.CUTOFF)
        columns = ac.compared_columns(con["depth"], von, bis, con["selected"], 1)
        out.append({"von": von, "bis": bis, "labels": labels, "con": con, "columns": columns,
                    "exp": ac.assign(rows, con["consensus"], von, columns)})
    return rows, text, mc, out


def quick_text(seed, rows, width):
    """a large random text over the full alphabet in a fraction of the time of cs_cases.random_msa: a quarter blank"""
    rng = np.random.default_rng(seed)
    table = np.frombuffer(b"acgtACGT-_  Nn  ", dtype=np.uint8)        # 16 entries: 10 symbols, 4 blanks, 2 other bytes
    text = table[rng.integers(0, 16, size=(rows, width), dtype=np.uint8)]
    text.setflags(write=False)
    return text


def random_codes(seed, parts, width):
    return np.random.default_rng(seed).integers(0, 5, size=(parts, width), dtype=np.uint8)
