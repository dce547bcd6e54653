"""-m gpu: the kernels behind MaxCorrelation, the group refinement, the subdivisions and the k-means stage on the deep
windows of tests/deep_cases.py -- more than 2 047 rows, so every loop over LDS chunks of 32 words runs a second (deep4160,
mc_ragged: a third) time, and a k-means part of more rows than one LDS tile holds -- against the checkers the small cases pin
to the reference (oracle/mc_oracle.c, tests/gr_checker.py, tests/sd_checker.py, tests/km_checker.py) and against what the
compiled reference wrote for the same inputs (tests/golden/rr_deep_reference.json.gz).

The comparisons are the existing ones, imported, with their bounds: _check of tests/test_gpu_max_correlation.py (zero pattern,
1e-9), compare of tests/test_gpu_group_refinement.py (exact arrays, drop_off 1e-12, no undecided variation allowed here),
compare of tests/test_gpu_subdivision.py (exact) and of tests/test_gpu_kmeans_subdivision.py (exact, every pair's Z 1e-9),
same of tests/test_gpu_window_reader.py (bit for bit).  tests/test_deep_windows.py asserts on the CPU what the cases rely on."""
import math

import numpy as np
import pytest

import deep_cases as dc
import gr_checker as gc
import rr_cases as rc
import sd_checker as sd
import test_gpu_group_refinement as t_gr
import test_gpu_kmeans_subdivision as t_km
import test_gpu_subdivision as t_sd
from test_gpu_max_correlation import _check
from test_gpu_window_reader import as_array, same
from test_subdivision import as_refined

pytestmark = pytest.mark.gpu


def mc_against_the_oracle(name, rows, mincov, exp):
    got, t = _check(rows, mincov, lambda _rows, _mincov: exp)
    T = len(rows)
    # the device and the host tail differ by the rounding of lgamma / exp / log10: about 3 ulp of lgamma(T + 1) in log10 units
    expected = 3 * 2.0 ** -53 * math.lgamma(T + 1) * math.log10(math.e)
    print(f"{name}: {T} rows (sc = {T // 64 + 1}), {int((exp > 0).sum())} non-zero values, {int((exp > 98).sum())} saturated, {t['pairs']} pairs, "
          f"largest |device - oracle| {float(np.abs(got - exp).max()):.3g} (rounding model {expected:.1g})")
    return got


@pytest.mark.parametrize("name", dc.DEEP_CASES)
def test_max_correlations_deep(name):
    rows, mc, von, bis, cov, _ = t_gr.checked(name)
    got = mc_against_the_oracle(name, rows, cov, mc)
    assert (got > 0).sum() > 500


@pytest.mark.parametrize("full_every", [0, 50])
def test_max_correlations_ragged_word_ranges(full_every):
    """read-like rows: the pairs' common word ranges start above word 0 and span more than one chunk (k_mc_pairs stages its
    second chunk from an unaligned wbeg); the twin with a full-width row every 50th: the ranges are all 69 words from word 0"""
    rows = dc.ragged_msa(full_every)
    got = mc_against_the_oracle("mc_ragged_full" if full_every else "mc_ragged", rows, dc.RAGGED_MINCOV, gc.mco_maxcorrs(rows, dc.RAGGED_MINCOV))
    assert (got > 98).sum() > 20 and ((got > 0) & (got < 98)).sum() > 1000


@pytest.mark.parametrize("name", dc.DEEP_CASES)
def test_refine_groups_deep(name):
    got, exp = t_gr.compare(name, max_undecided=0.0)
    kept = dc.DEEP_SEEDS[name][1]
    assert got.kept.sum() == kept and got.c_groups.shape[1] == kept // 64 + 1 > dc.CHUNK_WORDS - 1
    assert (exp["sizes"] > 5).sum() >= 40


@pytest.mark.parametrize("name", dc.DEEP_LABEL_CASES)
def test_subdivide_deep(name):
    got, exp, ref, win = t_sd.compare(name)
    assert got.dropoff_parts == 3 and got.eligible == 3 and got.selected > 0


@pytest.mark.parametrize("name", dc.DEEP_LABEL_CASES)
def test_kmeans_subdivide_deep_equals_the_checker_and_the_reference(name):
    """compare of tests/test_gpu_kmeans_subdivision.py: rows, vars, cluster numbers and labels exactly, every evaluated
    pair's Z within 1e-9, and the labels' text equal to the reference's KmeansSubdivisionOf_ file"""
    got, exp = t_km.compare(name, dc.checker_run(name))
    assert got.eligible == 3 and got.pairs > 1000


def test_kmeans_second_tile_and_second_block():
    """km_deep: a part of 520 rows with sc_km = 8 (tiles of 512 rows: k_km_centroids and k_km_assign refill their LDS tile
    and carry the five-slot list and the best score into it), more than 256 variations in the part (blockIdx.x > 0 of
    k_km_counts and k_km_pairs, many z blocks joined by the atomic maximum) and 33 words of rows"""
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide
    rows, win, ref, lab, exp = dc.km_deep()
    got = kmeans_subdivide(rows, as_refined(ref), lab, cov=dc.KM_DEEP_COV, debug_pairs=True)
    p = exp["eligible"][0]
    assert got.eligible == 1 and got.part == [p["part"]] and list(got.rows[0]) == p["rows"]
    worst = max(abs(got.pair_z[(0, i, j)] - z) for i, j, z in p["pairs"])
    print(f"km_deep: {len(p['rows'])} rows, varzahl {p['varzahl']}, {got.pairs} pairs, {len(p['moves'])} moves, largest |Z - checker| {worst:.3g}")
    assert len(got.pair_z) == got.pairs == len(p["pairs"]) and worst <= 1e-9
    assert list(got.vars[0]) == p["vars"]
    assert list(got.cluster_before[0]) == p["before"] and list(got.cluster_after[0]) == p["after"]
    assert got.parts == exp["parts"] and got.parts_before == exp["parts_before"] and np.array_equal(got.labels, exp["labels"])


def test_window_reader_deep():
    """pgr_msa_window against pgr_read_window at sc = 33: the 2 049th kept row is bit 0 of word 32"""
    from repeatresolver_amd.resolution import open_msa
    rows = dc.case_input("deep2049")["rows"]
    text = as_array(rows)
    with open_msa(rows) as msa:
        exp = same(msa, text, None, None)
    assert exp["kept_rows"] == 2049 and exp["sc"] == 33 and exp["rows"] == 2055
    assert np.bitwise_or.reduce(exp["local_coverage"][:, 32]) == 1 and np.bitwise_or.reduce(exp["groups"][:, 32]) == 1


def test_resolve_deep_equals_the_checker_chain():
    """resolution.resolve over the whole width of deep2049: the device reader's sets stay on the device and the refinement,
    the subdivisions and the k-means stage run on them; labels and part counts of the three checkers fed the same MaxCorrs"""
    from repeatresolver_amd.resolution import open_msa, resolve
    rec, _, case, win, ref, sub, kmr = dc.checker_run("deep2049")
    with open_msa(case["rows"]) as msa:
        got = resolve(msa, rc.maxcorrs_values(rec), [0, len(case["rows"][0]) - 1], case["cov"])
    assert len(got) == 1
    w = got[0]
    assert w.kept_rows == 2049 and w.cutoff == ref["cutoff"]
    assert np.array_equal(w.dropoff_labels, sub["dropoff_labels"]) and np.array_equal(w.reldrop_labels, sub["reldrop_labels"])
    assert np.array_equal(w.kmeans_labels, kmr["labels"])
    assert (w.dropoff_parts, w.reldrop_parts, w.kmeans_parts) == (sub["dropoff_parts"], sub["reldrop_parts"], kmr["parts"])


@pytest.mark.parametrize("name", dc.DEEP_LABEL_CASES)
def test_device_chain_against_the_reference_files(name):
    """the device's MaxCorrelation as the "%f" text of its file against the reference's (rr_cases.compare_maxcorrs_text), and
    from those six-decimal values the device's refinement, subdivisions and k-means: the reference's three label files"""
    from repeatresolver_amd.group_refinement import refine_groups
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide
    from repeatresolver_amd.max_correlation import max_correlations
    from repeatresolver_amd.subdivision import subdivide
    rec, case = dc.checked_input(name)
    rows, von, bis, cov = case["rows"], case["von"], case["bis"], case["cov"]
    lines = ["%f" % v for v in max_correlations(rows, cov)]
    differing = rc.compare_maxcorrs_text(lines, rc.maxcorrs_lines(rec))
    print(f"{name}: {differing} of {len(lines)} '%f' lines differ between device and reference")
    refined = refine_groups(rows, np.array([float(v) for v in lines]), von, bis, cov)
    sub = subdivide(rows, refined, von, bis, cov)
    kms = kmeans_subdivide(rows, refined, sub, von, bis, cov)
    assert sd.subdivision_bytes(sub.dropoff_labels) == rec["dropoff"]["text"].encode()
    assert sd.subdivision_bytes(sub.reldrop_labels) == rec["reldrop"]["text"].encode()
    assert sd.subdivision_bytes(kms.labels) == rec["kmeans"]["text"].encode()
