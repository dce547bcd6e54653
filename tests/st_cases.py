"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  The inputs tests/test_settle.py (no GPU) and tests/test_gpu_settle.py share: the
hand-made 6 x 9 case of tests/cs_cases.py with two iterations worked out by hand, the inputs A and B on the random text of the
consensus tests, the noisy-copies input C with its four variants, and what tests/st_checker.py gives for each (computed once
per process).  Everything compared is an integer: every comparison is exact."""
import functools

import numpy as np

import cs_cases as cs
import st_checker as st

# ---- the hand-made case: cs_cases.HAND_ROWS, every column of [0, 8], thresholds (3, 1), free ------------------------------
# Iteration 0 starts from HAND_LABELS = 0 0 2 2 - 2: the consensus is cs_cases.HAND_CONSENSUS, column 2 drops out (part 0 has
# depth 0 there), and as_cases works out the rows: compared 8 7 8 8 8 6, mismatches (0,4) (3,3) (2,2) (4,0) (6,6) (6,3).
# Margin >= 1 and compared >= 3: row 0 -> part 0 (label 0), rows 1, 2 and 4 tie (margin 0) -> -1, row 3 -> part 1 (label 2),
# row 5 -> part 1 (label 2).  New labels 0 - - 2 - 2: rows 1 and 2 moved, 2 changed.
# Iteration 1 starts from 0 - - 2 - 2: part 0 is row 0 alone, part 1 is rows 3 and 5.
#   column:       0    1    2    3    4    5    6    7    8
#   row 0         a    g    .    A    _    t    c    g    T      part 0 = 0 2 0 0 4 3 1 2 3, depth 1 1 0 1 1 1 1 1 1
#   row 3         C    g    T    c    _    t    g    -    t
#   row 5         c    -    -    c    a    .    a    -    .      part 1: c | g/- tie -> g | t/- tie -> t | c | a/- tie -> a | t | a/g tie -> a
#                                                                 | - | t  = 1 2 3 1 0 3 0 4 3, depth 2 2 2 2 2 1 2 2 1
# Column 2 drops out again.  Over 0 1 3 4 5 6 7 8, part 0 is a g a - t c g t and part 1 is c g c a t a - t:
#   row 0  a g A _ t c g T  (0, 5: columns 0 3 4 6 7)       row 1  c - a - t C - .  7 compared: part 0: 0 1 7; part 1: 1 3 4 6 -> (3, 4)
#   row 2  c g a - t g g t  part 0: 0 6; part 1: 3 4 6 7 -> (2, 4)    row 3  C g c _ t g - t  part 0: 0 3 6 7; part 1: 4 6 -> (4, 2)
#   row 4  t t t t t t t t  (6, 6)                           row 5  c - c a . a - .  6 compared: part 0: all six; part 1: column 1 -> (6, 1)
# New labels: 0, 0 (margin 1), 0 (margin 2), 2, - (a tie), 2: rows 1 and 2 moved again, 2 changed.  Iteration 2 (not written out)
# moves nothing: converged after three iterations with 0 0 0 2 - 2.
HAND_ARGS = dict(min_compared=3, min_margin=1, max_iter=2, all_columns=True)
HAND_COLUMNS = [0, 1, 3, 4, 5, 6, 7, 8]
HAND_LABELS_AFTER = [[0, -1, -1, 2, -1, 2], [0, 0, 0, 2, -1, 2]]
HAND_CHANGED = [2, 2]
HAND_COMPARED = [8, 7, 8, 8, 8, 6]
HAND_MISMATCHES_1 = [[0, 5], [3, 4], [2, 4], [4, 2], [6, 6], [6, 1]]      # of iteration 1
HAND_BEST_1 = [0, 0, 0, 1, 0, 1]
HAND_SECOND_1 = [1, 1, 1, 0, 1, 0]


def hand_labels():
    return np.array([-1 if x is None else x for x in cs.HAND_LABELS], dtype=np.int32)


# ---- A and B: cs_cases.random_msa(3, 900, 1031), window [0, 1030], the columns over the cutoff 1.0 ---------------------------
AB_ARGS = dict(min_compared=5, min_margin=1, max_iter=12)


def ab_text():
    return cs.random_msa(3, 900, 1031)


# ---- C: noisy copies -----------------------------------------------------------------------------------------------------
C_ROWS, C_WIDTH, C_COPIES = 900, 1031, 5
SYMBOLS = np.frombuffer(b"acgt-", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def noisy_copies(seed=24):
    """(text [900, 1031] uint8, truth [900] the copy of every row, seeds [900] int32: 2 * copy + 1 for 30 % of the rows, -1 for
    the others, MaxCorrs that select every third column over the cutoff 1.0).  Five copies of one random sequence that differ
    from it in 6 % of the columns each; every symbol of a row replaced by a random one of a c g t - with probability 0.15; 30 %
    of the symbols in upper case (gaps as '_'); every row blank before a random start in the first and behind a random end in the
    last third."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, C_WIDTH)
    copies = np.tile(base, (C_COPIES, 1))
    for c in range(C_COPIES):
        at = rng.choice(C_WIDTH, size=int(0.06 * C_WIDTH), replace=False)
        copies[c, at] = (copies[c, at] + rng.integers(1, 5, len(at))) % 5          # another symbol, a gap among them
    truth = rng.integers(0, C_COPIES, C_ROWS)
    codes = copies[truth]
    wrong = rng.random(codes.shape) < 0.15
    codes = np.where(wrong, rng.integers(0, 5, codes.shape), codes)
    text = SYMBOLS[codes]
    upper = rng.random(codes.shape) < 0.30
    text = np.where(upper, np.where(codes == 4, ord("_"), text - 32), text).astype(np.uint8)
    start, end = rng.integers(0, C_WIDTH // 3, C_ROWS), rng.integers(2 * C_WIDTH // 3, C_WIDTH + 1, C_ROWS)
    cols = np.arange(C_WIDTH)
    text[(cols < start[:, None]) | (cols >= end[:, None])] = ord(" ")
    seeds = np.where(rng.random(C_ROWS) < 0.30, 2 * truth + 1, -1).astype(np.int32)
    mc = np.zeros(C_WIDTH * 5)
    mc[5 * np.arange(0, C_WIDTH, 3) + 2] = 3.0
    text = np.ascontiguousarray(text)
    for a in (text, truth, seeds, mc):
        a.setflags(write=False)
    return text, truth, seeds, mc


def c_labels(variant):
    """the initial labelling of C1 .. C4"""
    text, truth, seeds, mc = noisy_copies()
    rng = np.random.default_rng(100 + variant)
    lab = seeds.copy()
    seeded = np.nonzero(seeds >= 0)[0]
    if variant == 1:                                                   # a quarter of the seeds on another copy
        bad = rng.choice(seeded, size=len(seeded) // 4, replace=False)
        lab[bad] = 2 * ((truth[bad] + rng.integers(1, C_COPIES, len(bad))) % C_COPIES) + 1
    elif variant == 2:                                                 # half of copy 0's seeds under a sixth label
        own = seeded[truth[seeded] == 0]
        lab[own[::2]] = 2 * C_COPIES + 1
    elif variant == 3:                                                 # a sixth label on one seeded row (the second) each of copies 0, 2 and 4
        for c in (0, 2, 4):
            lab[seeded[truth[seeded] == c][1]] = 2 * C_COPIES + 1
    return lab


# (variant, candidates, thresholds, hold, min_depth).  C2-depth2 is C2 with min_depth 2: it runs out of columns in its third
# iteration, so what it returns is the second's.
C_CASES = {"C1-free": (1, "all", (10, 1), False, 1), "C1-hold": (1, "all", (10, 1), True, 1), "C1-third-free": (1, "third", (10, 1), False, 1),
           "C2-free": (2, "all", (10, 1), False, 1), "C2-depth2": (2, "all", (10, 1), False, 2), "C3-free": (3, "all", (10, 0), False, 1),
           "C3-hold": (3, "all", (10, 0), True, 1), "C3-third-free": (3, "third", (10, 0), False, 1),
           "C4-free": (4, "all", (C_WIDTH + 1, 1), False, 1)}
C_MAX_ITER = 12


def c_args(name):
    variant, candidates, (min_compared, min_margin), hold, min_depth = C_CASES[name]
    text, truth, seeds, mc = noisy_copies()
    return c_labels(variant), dict(von=0, bis=C_WIDTH - 1, maxcorrs=mc if candidates == "third" else None, cutoff=1.0,
                                   min_compared=min_compared, min_margin=min_margin, max_iter=C_MAX_ITER, hold=hold, min_depth=min_depth)


def share_true(labels, truth):
    """(rows labelled, the share of them whose label is 2 * their copy + 1)"""
    inside = labels >= 0
    return int(inside.sum()), float((labels[inside] == 2 * truth[inside] + 1).mean())


@functools.lru_cache(maxsize=None)
def expected(name):
    """what st_checker.settle gives for the named case: "hand", "A-hold", "A-free", "B" or a key of C_CASES"""
    if name == "hand":
        return st.settle(cs.HAND_ROWS, hand_labels(), 0, 8, None, 1.0, plain=True, **HAND_ARGS)
    if name in ("A-hold", "A-free", "B"):
        text, mc = ab_text()
        labels = cs.many_parts_labels(900, 130) if name == "B" else cs.geometry_labels()
        return st.settle(text, labels, 0, 1030, mc, 1.0, hold=name == "A-hold", **AB_ARGS)
    labels, kw = c_args(name)
    return st.settle(noisy_copies()[0], labels, kw.pop("von"), kw.pop("bis"), kw.pop("maxcorrs"), kw.pop("cutoff"), **kw)
