"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The inputs and the fixture of the reference pinning of MaxCorrelation and RepeatResolver's first stages, shared by the
generator oracle/gen_rr_fixtures.py (which runs the compiled reference on them and writes tests/golden/rr_reference.json.gz)
and by tests/test_rr_reference.py / tests/test_gpu_rr_reference.py (which regenerate the inputs from their seeds, check
their sha256 against the fixture's and compare the checkers, the host pieces and the device with what the reference wrote).

Every case is a dict: rows (equally long byte strings), cov (the reference's -c), von / bis (its -f, None: the whole
width), labels (True: RepeatResolver ran on it and its two label files are compared exactly; False: MaxCorrelation only)."""
import functools
import gzip
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN
import gr_checker as gc
from test_gpu_group_refinement import CASES, checked, fixture_cases, planted_msa
from test_mc_oracle import small_msa
from test_subdivision import REL_CASES, synthetic

FIXTURE = os.path.join(GOLDEN, "rr_reference.json.gz")
MSA_NAME = "MSA"                                                    # the file name the reference ran on: part of its output names
MC_SHAPES = [(63, 300), (64, 300), (65, 300), (129, 900), (40, 2200)]   # test_word_and_tile_boundaries
STRETCH = 21                                                        # MaxCorrelation pairs columns at least 20 apart (MC:798)
DEEP_SEED = 38      # of the seeds 6 .. 39 tried: stage 2 splits the parts 79 and 171, the second and third pass of 64
# Three of the existing inputs hold one `undecided` variation each (kept64, kept65, rel5groups: two candidate values 1e-14
# apart at ranks 1 to 3 of 5 to 15).  Those inputs stay as they are -- the existing tests are built on them -- and each gets
# a sibling of the same shape with another seed and no undecided variation: name -> (rows, von, bis, cov), as CASES.
RESEEDED = {
    "kept64_reseeded": lambda: (planted_msa(164, 64, 300, [8, 8, 8]), None, None, 12),
    "kept65_reseeded": lambda: (planted_msa(165, 65, 300, [8, 8, 8]), None, None, 12),
    "rel5groups_reseeded": lambda: (planted_msa(13, 200, 450, [14, 8, 8, 6, 6], noise=0.25), None, None, 10),
}
KERNEL_TILE = 64                                                    # PGR_SD_TILE of pgr_device.hip: parts per pass of k_gr_reldrop


def stretched(seed=5):
    """synthetic(7) of tests/test_subdivision.py with every column moved to 21 x its index and 'a' in between: its planted
    families (7 neighbouring columns each) come to lie 21 columns apart, so the reference's own MaxCorrelation pairs them
    and its own Cliquer builds the cliques -- no hand-made arrays.  639 rows x 1554 columns, cov 2."""
    rows = synthetic(7, seed)[0]
    W = len(rows[0])
    out = []
    for r in rows:
        row = bytearray(b"a" * (STRETCH * W))
        row[::STRETCH] = r
        out.append(bytes(row))
    return out


def _case(rows, cov, von=None, bis=None, labels=True):
    return {"rows": rows, "cov": cov, "von": von, "bis": bis, "labels": labels}


def _realigned(name):
    rows, _mc, von, bis, cov, _exp = checked(name)                  # the 600-column middle, as checked() cuts it
    return _case(rows, cov, von, bis)


def _from_tuple(make):
    rows, von, bis, cov = make()                                    # the layout of CASES and REL_CASES
    return _case(rows, cov, von, bis)


def _builders():
    b = {}
    for name, make in list(CASES.items()) + list(REL_CASES.items()) + list(RESEEDED.items()):
        b[name] = functools.partial(_from_tuple, make)
    for name in fixture_cases():
        b["realigned_" + name] = lambda name=name: _realigned(name)
    b["stretched"] = lambda: _case(stretched(), 2)
    b["stretched_deep"] = lambda: _case(stretched(DEEP_SEED), 2)
    for T, W in MC_SHAPES:
        b[f"mc_{T}x{W}"] = lambda T=T, W=W: _case(small_msa(seed=T + W, T=T, W=W), 10, labels=False)
    for mincov in (4, 12, 30):
        b[f"mc_small_c{mincov}"] = lambda mincov=mincov: _case(small_msa(), mincov, labels=False)
    return b


BUILDERS = _builders()


@functools.lru_cache(maxsize=None)
def case_input(name):
    return BUILDERS[name]()


def msa_bytes(rows):
    return b"\n".join(rows) + b"\n"


def input_sha256(rows):
    return hashlib.sha256(msa_bytes(rows)).hexdigest()


@functools.lru_cache(maxsize=None)
def load_fixture():
    """{name: record} as oracle/gen_rr_fixtures.py wrote them"""
    with gzip.open(FIXTURE, "rb") as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def fixture_names(labels=None):
    """the names in the committed fixture (at collection time), all or by kind"""
    return [n for n, c in load_fixture().items() if labels is None or c["labels"] == labels]


def maxcorrs_lines(rec):
    """the lines of the reference's MaxCorrsOf_ file, rebuilt: "0.000000" wherever the fixture lists nothing"""
    lines = ["0.000000"] * rec["maxcorrs"]["lines"]
    for i, text in rec["maxcorrs"]["nonzero"]:
        lines[i] = text
    return lines


def maxcorrs_values(rec):
    return np.array([float(v) for v in maxcorrs_lines(rec)])


def checked_input(name):
    """the regenerated input of a fixture case; FAILS (never skips) when it is not the input the reference ran on"""
    rec, case = load_fixture()[name], case_input(name)
    assert input_sha256(case["rows"]) == rec["input_sha256"], f"{name}: the regenerated input differs from the fixture's"
    assert (case["cov"], case["von"], case["bis"], case["labels"]) == (rec["cov"], rec["von"], rec["bis"], rec["labels"])
    return rec, case


def clique_set_decided(cands, greedy, eps=1e-8):
    """For an `undecided` variation (gr_checker.undecided: a rounding difference of the tail could reorder its clique), still
    enough for exact labels: nothing within eps of the greedy threshold, at most 29 candidates above it (the cut at 30 drops
    none) and variation 0 not among them (its PLACE would end Sizes, RR:1650).  Then the clique is the same SET whatever the
    order, Sizes is its length, and every later step -- Dropoff_Cutoff, CliqueGroup, both subdivisions -- sums votes over
    that set (RR:976-1008, RR:1460-1522, RR:2859-2920): the labels do not depend on the order."""
    r = gc.ranked(cands, greedy)
    return not any(abs(z - greedy) < eps for z, _ in cands) and len(r) <= gc.MAXCLIQUE - 1 and all(i != 0 for _, i in r)


def label_conditions(case, rec, refined=None, near_cutoff=1e-5):
    """The conditions under which the labels of a case are compared exactly, from the input and the reference's MaxCorrs:
    returns ("strict": no undecided variation | "clique_sets": the undecided ones are clique_set_decided, number of
    significant variations, the undecided variations); fails when neither holds or a non-zero MaxCorrs value of the window
    lies within near_cutoff of the cutoff (the values have six decimals).  refined: (window, its refine()) if already made."""
    mc = maxcorrs_values(rec)
    win, exp = refined if refined else (None, None)
    if win is None:
        win = gc.Window(case["rows"], mc, case["von"], case["bis"], case["cov"])
        exp = win.refine()
    und = [s for s in range(len(exp["significant"])) if gc.undecided(exp["candidates"][s], exp["cutoff"])]
    loose = [int(exp["significant"][s]) for s in und if not clique_set_decided(exp["candidates"][s], exp["cutoff"])]
    assert not loose, f"{rec['name']}: variations {loose[:5]} whose clique a rounding difference could change: choose another seed"
    sliced = mc[win.von * 5:(win.bis + 1) * 5]                        # before the coverage restriction, as RR:3981 counts them
    nz = sliced[sliced != 0]
    near = float(np.abs(nz - win.cutoff).min()) if len(nz) else float("inf")
    assert near > near_cutoff, f"{rec['name']}: a MaxCorrs value {near} from the cutoff: choose another seed"
    return ("clique_sets" if und else "strict"), len(exp["significant"]), [int(exp["significant"][s]) for s in und]


def stdout_value(rec, prog, prefix):
    """the recorded stdout line of `prog` ("mc" / "rr") that starts with prefix"""
    hits = [l for l in rec["stdout"][prog] if l.startswith(prefix)]
    assert len(hits) == 1, (rec["name"], prog, prefix, hits)
    return hits[0]


def compare_maxcorrs_text(got_lines, ref_lines):
    """The three criteria of test_cli_writes_the_reference_file for two MaxCorrsOf_ texts: the zero pattern identical, the
    values within 1.5e-6, at most 0.5 % of the lines different as text.  Returns the number of differing lines."""
    assert len(got_lines) == len(ref_lines)
    got, ref = np.array([float(v) for v in got_lines]), np.array([float(v) for v in ref_lines])
    assert np.array_equal(got == 0, ref == 0)
    assert np.allclose(got, ref, rtol=0, atol=1.5e-6), float(np.abs(got - ref).max())
    differing = sum(a != b for a, b in zip(got_lines, ref_lines))
    assert differing <= 0.005 * len(ref_lines), (differing, len(ref_lines))
    return differing
