"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The inputs and the fixture of the reference pinning of RepeatResolver's k-means stage (Kmeans_Subdivision, RR:3382-3403),
shared by the generator scripts/gen_km_fixtures.py (which runs the compiled reference on them and writes
tests/golden/rr_kmeans_reference.json.gz) and by tests/test_kmeans_subdivision.py / tests/test_gpu_kmeans_subdivision.py.

The cases are the label cases of tests/rr_cases.py (their MaxCorrsOf_ lines and first two label files stay in
rr_reference.json.gz) plus the ones built here, the smallest shapes at which the stage can still go wrong.  The new inputs
carry no noise: a background of 'a' and marked columns in which named row groups hold other symbols.  What makes the stage
see anything at all is a group of EXACTLY mingroup = cov / 2 rows: both drop-off stages split only where more than mingroup
rows fall on either side (RR:3244, RR:3351), Relative_Vars keeps a variation held by at least mingroup rows of the part
(RR:2448).  Marked columns that are to correlate lie 21 apart (MaxCorrelation pairs columns at least 20 apart)."""
import functools
import gzip
import json
import os

import numpy as np

import rr_cases as rc
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "rr_kmeans_reference.json.gz")
STEP = 21


def marked_msa(T, W, groups, marks, seed=None):
    """T rows of W 'a'; marks = [(column, {group name: symbol}, symbol of the other rows)], a later group of the dict
    overrides an earlier one; groups = {name: rows}.  seed: the rows are shuffled (groups then straddle the 64-row words)."""
    text = np.full((T, W), ord("a"), dtype=np.uint8)
    for col, syms, rest in marks:
        text[:, col] = ord(rest)
        for g, s in syms.items():
            text[groups[g], col] = ord(s)
    if seed is not None:
        text = text[np.random.default_rng(seed).permutation(T)]
    return [bytes(r) for r in text]


def variables_case(T, double, odd, seed=None):
    """One part of T rows at cov 10 with one group of exactly 5 rows, A: `double` columns hold A against all the others (two
    variations each) and `odd` (0 or 1) column holds A against the others halved by the parity of the row, halves that
    correlate with nothing (one variation): varzahl = 2 * double + odd."""
    groups = {"A": list(range(5)), "even": list(range(6, T, 2))}
    marks = [(STEP * n, {"A": "c"}, "t") for n in range(double)]
    marks += [(STEP * (double + n), {"even": "g", "A": "c"}, "t") for n in range(odd)]
    return marked_msa(T, STEP * (double + odd), groups, marks, seed)


def small_parts(singles=False):
    """cov 2 on 40 rows: X (3 rows) and Y (4 rows) are split off by stage 1 and are eligible (more than 2 * mingroup = 2
    rows).  No pair of variations can reach the cutoff inside so small a part (at best -log10(1/6) in 4 rows), so the
    reference runs k-means there without variables.  singles: one row of X and one of Y marked on their own as well, for
    the hand-fed device test with a cutoff of 0.45 (tests/test_gpu_kmeans_subdivision.py)."""
    groups = {"X": [0, 1, 2], "Y": [3, 4, 5, 6], "x": [0], "y": [3]}
    marks = [(STEP * n, {"X": "c", "Y": "g"}, "t") for n in range(8)]
    if singles:
        marks += [(STEP * (8 + n), {"x": "c"}, "t") for n in range(6)] + [(STEP * (14 + n), {"y": "g"}, "t") for n in range(6)]
    return marked_msa(40, STEP * (20 if singles else 8), groups, marks)


def chain_case(cov, T, sizes, seed):
    """Groups of exactly mingroup rows that overlap: consecutive groups share sizes[n] rows, so the rows fall into classes
    of many sizes below mingroup, which the reassignment chain dissolves round after round."""
    m = cov // 2
    groups, start = {}, 0
    for n in range(len(sizes) + 1):
        groups[n] = list(range(start, start + m))
        if n < len(sizes):
            start += m - sizes[n]
    marks = []
    for n in groups:
        marks += [(STEP * (n * 8 + q), {n: "cg"[n % 2]}, "t") for q in range(8)]
    return marked_msa(T, STEP * 8 * len(groups), groups, marks, seed)


def distance_case(exactly_100):
    """40 rows at cov 10, A = 5 rows.  A is marked in the columns 0, 2 .. 9 and 20: only the columns 0 and 20 have a partner
    20 columns away, so only their variations have MaxCorrs; the others just fill the cliques (Sizes > 5, RR:1684).  Column
    0 holds g / t (indices 2, 3), column 20 a / c (100, 101): every pair is 97 to 99 apart and Relative_Vars (RR:2462)
    evaluates none.  The twin holds a / g in column 20 (100, 102): the pair (2, 102) is exactly 100 apart."""
    groups = {"A": list(range(5))}
    marks = [(0, {"A": "t"}, "g")] + [(c, {"A": "t"}, "c") for c in range(2, 10)]
    marks += [(20, {"A": "g" if exactly_100 else "c"}, "a")]
    return marked_msa(40, 40, groups, marks)


def _case(rows, cov, von=None, bis=None):
    return {"rows": rows, "cov": cov, "von": von, "bis": bis, "labels": True}


NEW_BUILDERS = {
    # varzahl 63, 64, 65 (sc_km 1 -> 2; 64: an all-zero second word) in parts of 63, 65 and 127 rows (row words 64 n +- 1)
    "km_vars63": lambda: _case(variables_case(63, 31, 1, seed=63), 10),
    "km_vars64": lambda: _case(variables_case(65, 32, 0, seed=64), 10),
    "km_vars65": lambda: _case(variables_case(127, 32, 1, seed=65), 10),
    "km_rows129": lambda: _case(variables_case(129, 8, 0, seed=129), 10),
    "km_small_parts": lambda: _case(small_parts(), 2),
    "km_chain_c30": lambda: _case(chain_case(30, 120, [4, 7, 2, 9, 5], seed=30), 30),
    "km_chain_c5": lambda: _case(chain_case(5, 100, [1, 1], seed=5), 5),
    "km_large": lambda: _case(variables_case(1100, 8, 1, seed=1100), 10),
    "km_distance_below": lambda: _case(distance_case(False), 10),
    "km_distance_100": lambda: _case(distance_case(True), 10),
}


@functools.lru_cache(maxsize=None)
def case_input(name):
    if name in NEW_BUILDERS:
        return NEW_BUILDERS[name]()
    return rc.case_input(name)


def case_names():
    return rc.fixture_names(labels=True) + list(NEW_BUILDERS)


def rr_args(case):
    """the reference's command line after the program name"""
    args = [rc.MSA_NAME, "-c", str(case["cov"])]
    if case["von"] is not None:
        args += ["-f", str(case["von"]), str(case["bis"])]
    return args


@functools.lru_cache(maxsize=None)
def load_fixture():
    with gzip.open(FIXTURE, "rb") as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def first_stages(name):
    """the record that holds a case's MaxCorrsOf_ lines and its first two label files: this fixture's for a new case,
    rr_reference.json.gz's otherwise"""
    return load_fixture()[name] if name in NEW_BUILDERS else rc.load_fixture()[name]


def checked_input(name):
    """(this fixture's record, the record of the first stages, the regenerated input); FAILS when the input is not the one
    the reference ran on"""
    rec, case = load_fixture()[name], case_input(name)
    assert rc.input_sha256(case["rows"]) == rec["input_sha256"], f"{name}: the regenerated input differs from the fixture's"
    assert rr_args(case) == rec["args"]
    return rec, first_stages(name), case
