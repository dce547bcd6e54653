"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The inputs tests/test_consensus.py (no GPU) and tests/test_gpu_consensus.py share:
the hand-made 6 x 9 case with its outcome worked out by hand, the main input's cutoff, the random inputs of the geometry tests
and the comparison of a resolution.Consensus with what tests/ta_checker.py gives.  Everything compared is an integer: every
comparison is exact."""
import functools

import numpy as np

import ta_checker as ta

KERNEL_TILE = 1024                                                    # PGR_CS_TILE of include/pgr.h: window columns per work-group of k_cs_counts
KERNEL_ROWS = 255                                                     # PGR_CS_ROWS: rows of one part per work-group
KERNEL_SCRATCH_INTS = 1 << 25                                         # PGR_CS_SCRATCH_INTS: count entries per range of columns
CUTOFF = 10.0                                                         # of the main input, ragged(31) of tests/test_gpu_resolve.py

# column:      0    1    2    3    4    5    6    7    8
HAND_ROWS = [b"ag A_tcgT",                                            # part 0
             b"c- a-tC- ",                                            # part 0
             b"cgta-tggt",                                            # part 2
             b"CgTc_tg-t",                                            # part 2
             b"ttttttttt",                                            # in no part: counted nowhere
             b"c--ca a- "]                                            # part 2
HAND_LABELS = [0, 0, 2, 2, None, 2]                                   # label 1 does not occur; None: an empty line of a label file (TA:74-75)
# part 0: a/c tie -> a | g/- tie -> g | depth 0 -> code 0 | A and a | _ and - | t t | c C | g/- tie -> g | T and a blank
# part 2: c C c | g g - | t T - | a c c | - _ a | t t and a blank | g g a | g - - | t t and a blank
HAND_CONSENSUS = [[0, 2, 0, 0, 4, 3, 1, 2, 3], [1, 2, 3, 1, 4, 3, 2, 4, 3]]
HAND_DEPTH = [[2, 2, 0, 2, 2, 2, 2, 2, 1], [3, 3, 3, 3, 3, 2, 3, 3, 2]]
HAND_SEQUENCES = [b"AGAATCGT", b"CGTCTGT"]                            # the '-' columns removed; the depth-0 column stays an A, as in the reference
HAND_DIFF_ALL = 5                                                     # columns 0 2 3 6 7
HAND_SELECTED = [0, 2, 3, 7, 8]                                       # column 1 sits exactly on the cutoff 1.0: not selected (TA:157 is >)
HAND_DIFF = 4                                                         # columns 0 2 3 7


def hand_maxcorrs():
    mc = np.zeros(45)
    for x in HAND_SELECTED:
        mc[5 * x + x % 5] = 2.0 + x
    mc[5 * 1 + 3] = 1.0
    mc[5 * 4: 5 * 4 + 5] = 0.999
    return mc


def same(con, exp, counts=True):
    """a resolution.Consensus against the dict of ta_checker.consensus, field by field, exactly"""
    assert (con.von, con.bis) == (exp["von"], exp["bis"])
    assert np.array_equal(con.part_label, exp["part_label"]) and np.array_equal(con.part_rows, exp["part_rows"])
    if counts:
        assert con.counts.shape == exp["counts"].shape and np.array_equal(con.counts, exp["counts"])
    assert con.consensus.shape == exp["consensus"].shape and np.array_equal(con.consensus, exp["consensus"])
    assert np.array_equal(con.depth, exp["depth"])
    assert np.array_equal(con.selected, exp["selected"])
    assert np.array_equal(con.diff, exp["diff"]) and np.array_equal(con.diff_all, exp["diff_all"])


ALPHABET = np.frombuffer(b"acgtACGT-_ Nn", dtype=np.uint8)            # the full alphabet: both cases, both gaps, blanks, other bytes


@functools.lru_cache(maxsize=None)
def random_msa(seed, rows, width, blank=0.25):
    """(uint8 array [rows, width], random MaxCorrs [width * 5]): a third of the columns over the cutoff 1.0, none near it"""
    rng = np.random.default_rng(seed)
    p = np.array([4, 4, 4, 4, 1, 1, 1, 1, 3, 1, 0, 0.5, 0.5])
    p = p / p.sum() * (1 - blank)
    p[10] = blank
    text = ALPHABET[rng.choice(len(ALPHABET), size=(rows, width), p=p)]
    mc = np.where(rng.random(width * 5) < 0.08, 2.0 + rng.random(width * 5), 0.5 * rng.random(width * 5))
    text.setflags(write=False)
    mc.setflags(write=False)
    return text, mc


def geometry_labels(rows=900):
    """one part of 2R + 1 rows, one of exactly R, one of a single row, the rest at -1; scattered over the rows, labels with gaps"""
    rng = np.random.default_rng(5)
    lab = np.full(rows, -1, dtype=np.int32)
    perm = rng.permutation(rows)
    R = KERNEL_ROWS
    lab[perm[:2 * R + 1]] = 1
    lab[perm[2 * R + 1:3 * R + 1]] = 4
    lab[perm[3 * R + 1]] = 9
    return lab


def many_parts_labels(rows, parts=130):
    """`parts` parts of one to five rows each (labels with gaps), the other rows at -1"""
    rng = np.random.default_rng(9)
    lab = np.full(rows, -1, dtype=np.int32)
    perm = rng.permutation(rows)
    at = 0
    for p in range(parts):
        n = 1 + p % 5
        lab[perm[at:at + n]] = 2 * p + 1
        at += n
    assert at <= rows
    return lab


def numpy_consensus(text, labels, von, bis):
    """The same integers from vectorised numpy, for inputs too large for the plain loops of ta_checker (the column ranges); it is
    itself compared with ta_checker on a small input in tests/test_consensus.py.  Returns (consensus, depth, diff_all)."""
    lut = np.full(256, 5, dtype=np.uint8)
    for ch, k in ta.INDEX.items():
        lut[ord(ch)] = k
    codes = lut[text[:, von:bis + 1]]
    found = [x for x in range(int(labels.max()) + 1) if (labels == x).any()]
    counts = np.stack([np.stack([(codes[labels == x] == k).sum(axis=0, dtype=np.int32) for k in range(5)], axis=1) for x in found])
    kon = counts.argmax(axis=2).astype(np.uint8)
    onehot = [(kon == k).astype(np.float32) for k in range(5)]
    equal = sum(o @ o.T for o in onehot)                              # (exact: integers far below 2^24)
    return kon, counts.sum(axis=2).astype(np.int32), (kon.shape[1] - equal).astype(np.int32)
