"""Runs without a GPU: what tests/test_gpu_deep_windows.py relies on.  The deep inputs of tests/deep_cases.py have the
structure that makes the kernels walk a second LDS chunk or tile (re-asserted here from the inputs and the checkers alone),
and the checkers reproduce what the REFERENCE wrote for deep2047 / deep2048 / deep2049 -- tests/golden/rr_deep_reference.json.gz,
recorded by oracle/gen_rr_fixtures.py --deep and scripts/gen_km_fixtures.py --deep from the unmodified MaxCorrelation.c and
RepeatResolver.c linked with the stand-in oracle/gsl_standin.c.  The inputs are regenerated from their seeds; a test FAILS
when the sha256 of its input is not the fixture's."""
import math

import numpy as np
import pytest

import deep_cases as dc
import gr_checker as gc
import km_checker as km
import rr_cases as rc
import sd_checker as sd
from test_gpu_group_refinement import CASES, checked
from test_subdivision import SD_CASES

MARGIN = 1e-8                                                       # of a k-means pair from the cutoff, as tests/test_kmeans_subdivision.py


def test_fixture_holds_data_only():
    fx = dc.load_fixture()
    assert list(fx) == dc.DEEP_LABEL_CASES
    for name, rec in fx.items():
        assert set(rec) == {"name", "cov", "von", "bis", "labels", "rows", "width", "input_sha256", "args", "stdout", "maxcorrs",
                            "condition", "dropoff", "reldrop", "kmeans"}
        assert rec["args"] == {"mc": [rc.MSA_NAME, "-c", "12", "-p", "1"], "rr": [rc.MSA_NAME, "-c", "12"]}
        assert rec["maxcorrs"]["lines"] == rec["width"] * 5 and all(text != "0.000000" for _, text in rec["maxcorrs"]["nonzero"])
        assert rc.stdout_value(rec, "mc", "There are ") == f"There are {rec['rows']} sequences."
        assert [rec[k]["file"] for k in ("dropoff", "reldrop", "kmeans")] == [f"{s}SubdivisionOf_0_1500000_MSA" for s in ("Dropoff", "RelDrop", "Kmeans")]
        assert rec["condition"] == "strict" and rec["rows"] == dc.DEEP_SEEDS[name][1] + 6


def test_the_deep_cases_stay_out_of_the_other_files_tables():
    """they go through checked() / sd_case() by name only: no parametrised test of the existing files runs on them"""
    assert not set(dc.DEEP_CASES) & (set(CASES) | set(SD_CASES) | set(rc.BUILDERS))


@pytest.mark.parametrize("name", dc.DEEP_LABEL_CASES)
def test_checkers_against_the_reference_files(name):
    """the oracle's MaxCorrs against the reference's file, the condition of the exact comparison, and the three label files
    byte for byte from the checkers fed the reference's MaxCorrs"""
    rec, _, case, win, ref, sub, got = dc.checker_run(name)
    differing = rc.compare_maxcorrs_text(["%f" % v for v in gc.mco_maxcorrs(case["rows"], case["cov"])], rc.maxcorrs_lines(rec))
    condition, sig, und = rc.label_conditions(case, rec, (win, ref))
    margin = km.margin(got["eligible"], win.cutoff)
    print(f"{name}: {differing} MaxCorrs lines differ, {sig} significant, {condition}, parts {sub['dropoff_parts']} -> {sub['reldrop_parts']} -> "
          f"{got['parts']}, k-means margin {margin:.3g}")
    assert condition == "strict" and und == [] and margin > MARGIN
    assert sd.subdivision_bytes(sub["dropoff_labels"]) == rec["dropoff"]["text"].encode()
    assert sd.subdivision_bytes(sub["reldrop_labels"]) == rec["reldrop"]["text"].encode()
    assert sd.subdivision_bytes(got["labels"]) == rec["kmeans"]["text"].encode()
    assert rc.stdout_value(rec, "rr", "Of ") == f"Of {len(case['rows'])} sequences, {win.T} had full coverage."


def deep_structure(name, win_T, exp):
    """what every deep refinement input must have: the word count, refined variations, both branches of the tail among the
    ranked candidates, and the last kept row in some refined group (2 048 rows: the last word exists and is empty)"""
    kept = dc.DEEP_SEEDS[name][1]
    sc = kept // 64 + 1
    assert win_T == kept and exp["c_groups"].shape[1] == sc and sc >= dc.CHUNK_WORDS
    assert (exp["sizes"] > 5).sum() >= 40
    sat, unsat = dc.tail_branches(exp)
    assert sat >= 300 and unsat >= 200
    last = np.bitwise_or.reduce(exp["c_groups"][:, (kept - 1) // 64])
    assert (int(last) >> ((kept - 1) % 64)) & 1
    if kept % 64 == 0:
        assert not exp["c_groups"][:, sc - 1].any() and not exp["c_coverage"][:, sc - 1].any()


@pytest.mark.parametrize("name", dc.DEEP_LABEL_CASES)
def test_structure_of_the_label_cases(name):
    """sc = 32, 33 with an empty last word, 33 with bit 0 of word 32; three parts, all eligible for k-means, every part with
    rows in the last word that holds any"""
    rec, _, case, win, ref, sub, got = dc.checker_run(name)
    deep_structure(name, win.T, ref)
    assert [dc.DEEP_SEEDS[n][1] // 64 + 1 for n in dc.DEEP_LABEL_CASES] == [32, 33, 33]
    assert sub["dropoff_parts"] == 3 and sub["selected"] > 0
    sizes = np.bincount(sub["reldrop_labels"][ref["kept"]])
    assert len(got["eligible"]) == len(sizes) == 3 and sizes.min() > win.T // 3 - 2
    assert sum(len(p["pairs"]) for p in got["eligible"]) > 1000
    assert not any(math.isnan(z) for p in got["eligible"] for _, _, z in p["pairs"])


def test_structure_of_the_three_chunk_case():
    """deep4160: sc = 66, and no undecided variation by the oracle's MaxCorrs (the GPU comparison allows none)"""
    rows, mc, von, bis, cov, exp = checked("deep4160")
    deep_structure("deep4160", int(exp["kept"].sum()), exp)
    assert exp["c_groups"].shape[1] == 66 > 2 * dc.CHUNK_WORDS
    assert not [s for s in range(len(exp["significant"])) if gc.undecided(exp["candidates"][s], exp["cutoff"])]
    assert (mc > 0).sum() > 500


def test_ragged_word_ranges():
    """mc_ragged: from the input alone, pairs of columns that MaxCorrelation evaluates whose common word range starts above
    word 0 and spans more than one chunk of 32 words; one full-width row would put every range's start at word 0, which is
    what the twin does on purpose: there every range starts at word 0 and most are all 69 words"""
    rows = dc.ragged_msa()
    assert len(rows) == 4400 and len(rows[0]) == 500 and len(rows) // 64 + 1 == 69
    assert not any(r[0] != 32 and r[-1] != 32 for r in rows)          # no row spans the width
    pairs, cols, longest = dc.deep_pairs(rows, dc.RAGGED_MINCOV)
    print(f"mc_ragged: {pairs} evaluated column pairs from {cols} columns start above word 0 and span more than 32 words (longest {longest})")
    assert pairs >= 1000 and cols >= 90 and longest > 2 * dc.CHUNK_WORDS
    twin = dc.ragged_msa(50)
    assert sum(r[0] != 32 and r[-1] != 32 for r in twin) == 88
    lo, hi, _ = dc.column_word_ranges(twin)
    assert (lo == 0).all() and (hi == 69).sum() >= 300 and dc.deep_pairs(twin, dc.RAGGED_MINCOV)[0] == 0
    pairs, cols, longest = dc.deep_pairs(twin, dc.RAGGED_MINCOV, from_word_0=True)
    assert pairs >= 1000 and longest == 69
    for r in (rows, twin):
        mc = gc.mco_maxcorrs(r, dc.RAGGED_MINCOV)
        assert (mc > 98).sum() > 20 and ((mc > 0) & (mc < 98)).sum() > 1000      # both branches of the significance


def test_km_deep_structure():
    """km_deep: sc_km >= 8, more rows in the part than one LDS tile holds, more than 256 variations in the part, rows of the
    part in the second chunk of words, a reassignment chain that moves rows, no NaN pair and none near the cutoff"""
    rows, win, ref, lab, exp = dc.km_deep()
    assert win.T == len(rows) == 2112 and win.T // 64 + 1 == 34 > dc.CHUNK_WORDS
    assert len(exp["eligible"]) == 1 and exp["parts_before"] == 161
    p = exp["eligible"][0]
    sc_km = p["varzahl"] // 64 + 1
    in_part = (lab == 0).astype(np.int64)
    marked = int(((ref["maxcorrs"] > ref["cutoff"]) & (win.G @ in_part >= dc.KM_DEEP_COV // 2)).sum())
    margin = km.margin([p], win.cutoff)
    print(f"km_deep: {len(p['rows'])} rows, varzahl {p['varzahl']} (sc_km {sc_km}, tiles of {dc.KM_TILE_WORDS // sc_km} rows), {marked} variations "
          f"in the part, {len(p['pairs'])} pairs, {len(p['moves'])} moves, margin {margin:.3g}, {sum(r >= 2048 for r in p['rows'])} rows from 2048 on")
    assert sc_km >= 8 and len(p["rows"]) == 520 > dc.KM_TILE_WORDS // sc_km
    assert marked > dc.KM_THREADS and len(p["pairs"]) > 100000
    assert margin > MARGIN and not any(math.isnan(z) for _, _, z in p["pairs"])
    assert sum(r >= 64 * dc.CHUNK_WORDS for r in p["rows"]) >= 5 and len({r // 64 for r in p["rows"]}) == 33     # every word that holds rows
    assert len(p["moves"]) > 0 and p["before"] != p["after"]
    # the second tile decides: for many rows i a row j of the second tile scores above the fifth best of the first tile, so it
    # enters i's five-slot list (RR:2682) and votes in i's centroid
    tile = dc.KM_TILE_WORDS // sc_km
    sigs = win.G[p["vars"]][:, p["rows"]].T
    own = km.match_matrix(sigs, sigs, sc_km)
    fifth = np.sort(own[:, :tile], axis=1)[:, -5]
    assert int((own[:, tile:].max(axis=1) > fifth).sum()) >= 20
