"""-m gpu: pgr_kmeans_subdivide (include/pgr.h; the kernels of pgr_km_device.hip) against the literal restatement
tests/km_checker.py and against the KmeansSubdivisionOf_ files of the reference (tests/golden/rr_kmeans_reference.json.gz).
Vars, Clusternumber before and after the chain and the labels are integers and compared exactly; the debug Z of every
evaluated pair within 1e-9 of the checker's (device and host tails differ only by rounding).

The device is fed the CHECKER's refined arrays and labels, as tests/test_gpu_subdivision.py does: the earlier stages' own
near-ties stay out of this comparison.  Inputs and their structure: tests/test_kmeans_subdivision.py."""
import os
import subprocess

import numpy as np
import pytest

import gr_checker as gc
import km_cases as kc
import km_checker as km
import rr_cases as rc
import sd_checker as sd
from test_kmeans_subdivision import CASES, CLI, checker_run
from test_subdivision import as_refined


def compare(name, run=None):
    """run: the tuple of checker_run for an input of another fixture (tests/deep_cases.py)"""
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide
    rec, first, case, win, ref, sub, exp = run or checker_run(name)
    got = kmeans_subdivide(case["rows"], as_refined(ref), sub["reldrop_labels"], case["von"], case["bis"], case["cov"], debug_pairs=True)
    parts = exp["eligible"]
    worst = 0.0
    assert got.part == [p["part"] for p in parts] and got.parts_before == exp["parts_before"]
    for e, p in enumerate(parts):
        assert list(got.rows[e]) == p["rows"]
        for i, j, z in p["pairs"]:
            worst = max(worst, abs(got.pair_z[(e, i, j)] - z))
    print(f"{name}: {got.eligible} eligible parts, {got.pairs} pairs, largest |Z - checker| {worst:.3g}")
    assert len(got.pair_z) == got.pairs == sum(len(p["pairs"]) for p in parts)
    assert worst <= 1e-9
    for e, p in enumerate(parts):
        assert list(got.vars[e]) == p["vars"], (name, e)
        assert list(got.cluster_before[e]) == p["before"], (name, e)
        assert list(got.cluster_after[e]) == p["after"], (name, e)
    assert got.parts == exp["parts"] and np.array_equal(got.labels, exp["labels"])
    assert sd.subdivision_bytes(got.labels) == rec["kmeans"]["text"].encode()
    return got, exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_equals_the_checker_and_the_reference(name):
    compare(name)


@pytest.mark.gpu
def test_small_parts_with_variables():
    """parts of 3 and of 4 rows whose single marked rows are variables: only a cutoff below -log10(1/3) lets a pair inside so
    small a part pass, so the window is fed by hand (every variation's MaxCorrs 1.0, cutoff 0.45, the labels X / Y / others)
    and compared with the checker alone.  Fewer than 5 rows: the initial top-5 slots survive."""
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide
    rows = kc.small_parts(singles=True)
    win = gc.Window(rows, np.ones(len(rows[0]) * 5), cov=2, cutoff=0.45)
    ref = {"maxcorrs": np.where(win.gsize > 0, 1.0, 0.0), "cutoff": 0.45, "kept": win.kept, "width": win.w, "significant": np.zeros(0, dtype=np.int32),
           "sizes": np.zeros(0, dtype=np.int32), "cliques": np.zeros((0, gc.MAXCLIQUE + 1), dtype=np.int32), "cutoffs": np.zeros(0, dtype=np.int32),
           "drop_off": np.zeros(0), "c_groups": np.zeros((0, win.T // 64 + 1), dtype=np.uint64), "c_coverage": np.zeros((0, win.T // 64 + 1), dtype=np.uint64)}
    lab = np.array([0] * 3 + [1] * 4 + [2] * 33, dtype=np.int32)
    exp = km.clustered(win, ref, lab, 2)
    assert [len(p["rows"]) for p in exp["eligible"]] == [3, 4, 33] and all(p["varzahl"] > 0 for p in exp["eligible"][:2])
    assert km.margin(exp["eligible"], 0.45) > 1e-8
    got = kmeans_subdivide(rows, as_refined(ref), lab, cov=2, debug_pairs=True)
    for e, p in enumerate(exp["eligible"]):
        assert list(got.vars[e]) == p["vars"] and list(got.cluster_before[e]) == p["before"] and list(got.cluster_after[e]) == p["after"]
        assert all(abs(got.pair_z[(e, i, j)] - z) <= 1e-9 for i, j, z in p["pairs"])
    assert np.array_equal(got.labels, exp["labels"])


@pytest.mark.gpu
def test_pipeline_chain():
    """pipeline.clustered end to end on the device (its own MaxCorrelation and refinement) against the reference's three files"""
    from repeatresolver_amd.kmeans_subdivision import last_timing
    from repeatresolver_amd.pipeline import clustered
    rec, first, case, win, ref, sub, exp = checker_run("km_vars65")
    s, k = clustered(case["rows"], case["von"], case["bis"], case["cov"])
    assert sd.subdivision_bytes(s.reldrop_labels) == first["reldrop"]["text"].encode()
    assert sd.subdivision_bytes(k.labels) == rec["kmeans"]["text"].encode() and [len(v) for v in k.vars] == [65]
    assert last_timing()["pairs_ms"] > 0 and last_timing()["pairs"] == k.pairs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rel5groups_reseeded", "window"])
def test_drop_in_binary_writes_the_reference_files(name, tmp_path):
    rec, first, case, win, ref, sub, exp = checker_run(name)
    (tmp_path / rc.MSA_NAME).write_bytes(rc.msa_bytes(case["rows"]))
    (tmp_path / ("MaxCorrsOf_" + rc.MSA_NAME)).write_text("".join(l + "\n" for l in rc.maxcorrs_lines(first)))
    p = subprocess.run([CLI] + rec["args"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-500:]
    for want in (first["dropoff"], first["reldrop"], rec["kmeans"]):
        assert (tmp_path / want["file"]).read_bytes() == want["text"].encode(), want["file"]
    assert sorted(n for n in os.listdir(tmp_path) if "SubdivisionOf_" in n) == sorted(w["file"] for w in (first["dropoff"], first["reldrop"], rec["kmeans"]))
