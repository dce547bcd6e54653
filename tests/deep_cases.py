"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The "deep windows": inputs with more than 2 047 rows, at which every kernel behind MaxCorrelation, the group refinement and
the k-means stage walks its row sets in more than one LDS chunk of 32 words (2 048 rows), and a hand-fed part whose rows
need more than one LDS tile of the k-means kernels.  Shared by tests/test_deep_windows.py (no GPU: the conditions the GPU
tests rely on, and the checkers against the reference's files), tests/test_gpu_deep_windows.py and the two fixture
generators (oracle/gen_rr_fixtures.py --deep, scripts/gen_km_fixtures.py --deep), which record what the compiled reference
writes for DEEP_LABEL_CASES in tests/golden/rr_deep_reference.json.gz.

  deep2047 / deep2048 / deep2049   planted_msa(seed, kept, 300, [8, 8, 8]), cov 12: sc = 32 (exactly one chunk), 33 with an
                                   all-zero last word, 33 with bit 0 of word 32 set
  deep4160                         the same generator at 160 columns, sc = 66: three chunks (MaxCorrelation and refinement
                                   only; at 300 columns the refinement checker alone needs 14 s, at 160 it needs 5)
  mc_ragged / mc_ragged_full       4 400 read-like rows over 500 columns for MaxCorrelation's word ranges (ragged_msa)
  km_deep                          2 112 rows x 230 columns, fed to the k-means stage by hand (km_deep)"""
import functools
import gzip
import json
import os

import numpy as np

import gr_checker as gc
import km_checker as km
import rr_cases as rc
import sd_checker as sd
from conftest import GOLDEN
from test_gpu_group_refinement import EXTRA_CASES, planted_msa

FIXTURE = os.path.join(GOLDEN, "rr_deep_reference.json.gz")
CHUNK_WORDS = 32                                                    # PMC_WC, PGR_WC, PKM_WC: words per LDS chunk
KM_TILE_WORDS = 4096                                                # PKM_LDS_WORDS: a tile of the k-means kernels holds 4096 / sc_km rows
KM_THREADS = 256                                                    # PKM_NT: variations per block of k_km_pairs and k_km_counts

# name -> (seed, kept rows, columns); with these seeds (the row counts: the first ones tried) the reference's MaxCorrs give
# rr_cases.label_conditions == "strict" and no k-means pair lies within 1e-8 of the cutoff
DEEP_SEEDS = {"deep2047": (2047, 2047, 300), "deep2048": (2048, 2048, 300), "deep2049": (2049, 2049, 300), "deep4160": (4160, 4160, 160)}
DEEP_LABEL_CASES = ["deep2047", "deep2048", "deep2049"]             # recorded with the reference, all three stages
DEEP_CASES = DEEP_LABEL_CASES + ["deep4160"]
DEEP_COV = 12

# name -> (rows, von, bis, cov), the layout of CASES of tests/test_gpu_group_refinement.py: checked() / compare() there and
# sd_case() of tests/test_subdivision.py find them, the parametrised tests of those files do not
for _name, (_seed, _kept, _W) in DEEP_SEEDS.items():
    EXTRA_CASES[_name] = lambda seed=_seed, kept=_kept, W=_W: (planted_msa(seed, kept, W, [8, 8, 8]), None, None, DEEP_COV)


@functools.lru_cache(maxsize=None)
def case_input(name):
    rows, von, bis, cov = EXTRA_CASES[name]()
    return {"rows": rows, "cov": cov, "von": von, "bis": bis, "labels": True}


# ---------------------------------------------------------------------------------------------------------------------------
# MaxCorrelation: read-like rows, so that the rows of a column sit in a range of words that starts above word 0
RAGGED_MINCOV = 30


@functools.lru_cache(maxsize=None)
def ragged_msa(full_every=0, T=4400, W=500, run=320, seed=44):
    """T rows over W columns; every row covers one run of about `run` columns from a random start and is blank elsewhere, so
    no row spans the width.  Three copy groups (row r: r % 3); every 11th column is a variant column in which one group,
    (column / 11) % 3, holds another base -- the variant columns of a group are linked.  3 % substitutions, 4 % gaps.
    full_every = n: every n-th row covers the whole width instead (the twin: every column's range then starts at word 0)."""
    rng = np.random.default_rng(seed)
    cons = rng.integers(0, 4, W)
    acgt = np.frombuffer(b"acgt", dtype=np.uint8)
    rows = []
    for r in range(T):
        seq = cons.copy()
        var = np.arange(5, W, 11)
        mine = var[(var // 11) % 3 == r % 3]
        seq[mine] = (cons[mine] + 1 + r % 3) % 4
        sub = rng.random(W) < 0.03
        seq[sub] = rng.integers(0, 4, int(sub.sum()))
        row = acgt[seq].copy()
        row[rng.random(W) < 0.04] = ord("-")
        a = int(rng.integers(0, W - run + 1))
        b = a + run + int(rng.integers(-20, 21))
        if full_every and r % full_every == 0:
            a, b = 0, W
        row[:a] = ord(" ")
        row[min(b, W):] = ord(" ")
        rows.append(row.tobytes())
    return rows


def column_word_ranges(rows):
    """What k_mc_bits / k_mc_colrange make of an input, from the input alone: the rows take their bit positions in the order
    of their first covered column (a stable sort), 64 per word; per column [lo, hi) = the words that hold a covering row.
    Returns (lo[W], hi[W], covered[T positions, W] as 0/1)."""
    text = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]))
    known = np.zeros(256, dtype=bool)
    known[list(gc._CODE)] = True
    covered = known[text]
    T, W = covered.shape
    start = np.where(covered.any(axis=1), covered.argmax(axis=1), W)
    covered = covered[np.argsort(start, kind="stable")]
    lo, hi = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
    for c in range(W):
        pos = np.flatnonzero(covered[:, c])
        if len(pos):
            lo[c], hi[c] = pos[0] // 64, pos[-1] // 64 + 1
    return lo, hi, covered.astype(np.int64)


def deep_pairs(rows, mincov, from_word_0=False):
    """The pairs of columns (ii, jj) that MaxCorrelation evaluates (jj >= ii + 20, every column from ii + 20 to jj shares at
    least mincov rows with ii, MC:798-804) whose common word range starts above word 0 (from_word_0: at word 0) and spans
    more than one LDS chunk: (number of such pairs, number of columns in one, the longest common range in words)."""
    lo, hi, covered = column_word_ranges(rows)
    shared = covered.T @ covered
    W = len(lo)
    pairs, cols, longest = 0, set(), 0
    for ii in range(W):
        for jj in range(ii + 20, W):
            if shared[ii, jj] < mincov:
                break
            beg, end = max(lo[ii], lo[jj]), min(hi[ii], hi[jj])
            if (beg > 0) != from_word_0 and end - beg > CHUNK_WORDS:
                pairs += 1
                cols.update((ii, jj))
                longest = max(longest, int(end - beg))
    return pairs, len(cols), longest


# ---------------------------------------------------------------------------------------------------------------------------
# k-means: one part of 520 rows with more than 448 variables, fed by hand
KM_DEEP_COV = 10


@functools.lru_cache(maxsize=None)
def km_deep(seed=1, T=2112, W=230, part_rows=520):
    """(rows, window, refined arrays, kept-row labels, the checker's result).  Five row groups (row r: r % 5); column c marks
    the group c % 5 ('c' against 't'); 4 % random substitutions.  Every variation with members gets MaxCorrs 50, the cutoff
    is the default.  520 rows drawn over all words are part 0; the others lie in parts of at most 10 = 2 * mingroup rows,
    which are not eligible."""
    rng = np.random.default_rng(seed)
    text = np.full((T, W), ord("t"), dtype=np.uint8)
    text[np.arange(T)[:, None] % 5 == np.arange(W)[None, :] % 5] = ord("c")
    sub = rng.random((T, W)) < 0.04
    text[sub] = np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    rows = [bytes(r) for r in text]
    win = gc.Window(rows, np.full(W * 5, 50.0), cov=KM_DEEP_COV)
    ref = {"maxcorrs": np.where(win.gsize > 0, 50.0, 0.0), "cutoff": win.cutoff, "kept": win.kept, "width": win.w,
           "significant": np.zeros(0, dtype=np.int32), "sizes": np.zeros(0, dtype=np.int32),
           "cliques": np.zeros((0, gc.MAXCLIQUE + 1), dtype=np.int32), "cutoffs": np.zeros(0, dtype=np.int32), "drop_off": np.zeros(0),
           "c_groups": np.zeros((0, win.T // 64 + 1), dtype=np.uint64), "c_coverage": np.zeros((0, win.T // 64 + 1), dtype=np.uint64)}
    part0 = np.sort(rng.choice(T, part_rows, replace=False))
    lab = np.zeros(T, dtype=np.int32)
    rest = np.setdiff1d(np.arange(T), part0)
    lab[rest] = 1 + np.arange(len(rest)) // 10
    return rows, win, ref, lab, km.clustered(win, ref, lab, KM_DEEP_COV)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's record of DEEP_LABEL_CASES
@functools.lru_cache(maxsize=None)
def load_fixture():
    """{name: record}: the record of oracle/gen_rr_fixtures.py (MaxCorrsOf_ lines, stdout lines, the first two label files)
    with the "kmeans" entry of scripts/gen_km_fixtures.py (the third label file)"""
    with gzip.open(FIXTURE, "rb") as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def checked_input(name):
    """(record, regenerated input); FAILS (never skips) when the input is not the one the reference ran on"""
    rec, case = load_fixture()[name], case_input(name)
    assert rc.input_sha256(case["rows"]) == rec["input_sha256"], f"{name}: the regenerated input differs from the fixture's"
    assert (case["cov"], case["von"], case["bis"], case["labels"]) == (rec["cov"], rec["von"], rec["bis"], rec["labels"])
    return rec, case


@functools.lru_cache(maxsize=None)
def checker_run(name):
    """The tuple of checker_run of tests/test_kmeans_subdivision.py -- (record, record of the first stages, case, window,
    refined arrays, subdivision, k-means result) -- by the three checkers fed the REFERENCE's MaxCorrs values; one record
    holds all stages here.  Once per process."""
    rec, case = checked_input(name)
    win = gc.Window(case["rows"], rc.maxcorrs_values(rec), case["von"], case["bis"], case["cov"])
    ref = win.refine()
    sub = sd.subdivide(win, ref, case["cov"])
    return rec, rec, case, win, ref, sub, km.clustered(win, ref, sub["reldrop_labels"], case["cov"])


def tail_branches(exp):
    """(saturated, unsaturated) values among the first 29 of the ranked candidate lists of a refine() result"""
    sat = unsat = 0
    for cands in exp["candidates"]:
        top = [z for z, _ in gc.ranked(cands, exp["cutoff"])[:gc.MAXCLIQUE - 1]]
        sat += sum(z > 97.9 for z in top)
        unsat += sum(z <= 97.9 for z in top)
    return sat, unsat
