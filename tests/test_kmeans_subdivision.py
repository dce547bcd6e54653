"""Runs without a GPU: the literal restatement of RepeatResolver's k-means stage (tests/km_checker.py) against what the
REFERENCE wrote -- tests/golden/rr_kmeans_reference.json.gz, recorded by scripts/gen_km_fixtures.py from the unmodified
RepeatResolver.c linked with the stand-in oracle/gsl_standin.c -- and the host pieces of the stage behind include/pgr.h.

The inputs are regenerated from their seeds (tests/rr_cases.py, tests/km_cases.py); a test FAILS when the sha256 of its input
is not the fixture's.  Condition of the exact comparison, re-asserted here: the label conditions of rr_cases.label_conditions
and no evaluated pair's Z within 1e-8 of the cutoff (the margin gr_checker.undecided uses for the same tail rounding)."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import gr_checker as gc
import km_cases as kc
import km_checker as km
import rr_cases as rc
import sd_checker as sd
from conftest import ROOT

CASES = kc.case_names()
MARGIN = 1e-8
CLI = os.path.join(ROOT, "repeatresolver_amd", "csrc", "RepeatResolver")


@functools.lru_cache(maxsize=None)
def checker_run(name):
    """(fixture record, record of the first stages, case, window, refined arrays, subdivision, k-means result by the checkers),
    fed the REFERENCE's MaxCorrs values; the existing cases share the run of tests/test_rr_reference.py"""
    rec, first, case = kc.checked_input(name)
    if name in kc.NEW_BUILDERS:
        win = gc.Window(case["rows"], rc.maxcorrs_values(first), case["von"], case["bis"], case["cov"])
        ref = win.refine()
        sub = sd.subdivide(win, ref, case["cov"])
    else:
        from test_rr_reference import checker_run as first_run
        _, _, win, ref, sub = first_run(name)
    return rec, first, case, win, ref, sub, km.clustered(win, ref, sub["reldrop_labels"], case["cov"])


def _lib():
    subprocess.run(["make", "-C", os.path.join(ROOT, "repeatresolver_amd", "csrc"), "all"], check=True, stdout=subprocess.DEVNULL)
    from repeatresolver_amd import _lib
    return _lib.load()


def test_fixture_holds_the_cases_it_must():
    fx = kc.load_fixture()
    assert set(rc.fixture_names(labels=True)) | set(kc.NEW_BUILDERS) == set(fx) and len(rc.fixture_names(labels=True)) == 31
    with __import__("gzip").open(kc.FIXTURE) as f:
        assert __import__("json").load(f)["vars_only"] == []         # no existing input misses the condition (at most 2 might)
    for name in kc.NEW_BUILDERS:
        assert fx[name]["maxcorrs"]["lines"] == fx[name]["width"] * 5 and fx[name]["dropoff"]["file"].startswith("DropoffSubdivisionOf_")
    assert fx["window"]["kmeans"]["file"] == "KmeansSubdivisionOf_120_330_MSA" and fx["kept63"]["kmeans"]["file"] == "KmeansSubdivisionOf_0_1500000_MSA"


@pytest.mark.parametrize("name", CASES)
def test_checker_against_the_reference_file(name):
    rec, first, case, win, ref, sub, got = checker_run(name)
    if name in kc.NEW_BUILDERS:
        assert rc.label_conditions(case, first, (win, ref))[0] == "strict"
        assert sd.subdivision_bytes(sub["dropoff_labels"]) == rec["dropoff"]["text"].encode()
        assert sd.subdivision_bytes(sub["reldrop_labels"]) == rec["reldrop"]["text"].encode()
    margin = km.margin(got["eligible"], win.cutoff)
    print(f"{name}: parts {got['parts_before']} -> {got['parts']}, varzahl {[p['varzahl'] for p in got['eligible']][:6]}, margin {margin:.3g}")
    assert margin > MARGIN
    assert sd.subdivision_bytes(got["labels"]) == rec["kmeans"]["text"].encode()
    assert sd.subdivision_name("Kmeans", case["von"], case["bis"], rc.MSA_NAME) == rec["kmeans"]["file"]


def test_structure_of_the_new_cases():
    """what the GPU tests rely on"""
    def parts(name):
        return checker_run(name)[6]["eligible"]
    assert [parts(n)[0]["varzahl"] for n in ("km_vars63", "km_vars64", "km_vars65")] == [63, 64, 65]
    assert [len(parts(n)[0]["rows"]) for n in ("km_vars63", "km_vars64", "km_vars65", "km_rows129")] == [63, 65, 127, 129]
    assert sorted(len(p["rows"]) for p in parts("km_small_parts")) == [3, 4, 33]
    # zero variables: every eligible part of `stretched` (3 to 6 rows at cov 2: no pair can reach the cutoff inside)
    st = parts("stretched")
    assert len(st) == 128 and all(p["varzahl"] == 0 for p in st) and 3 <= min(len(p["rows"]) for p in st) < 5
    assert all(p["before"] == [1] + [0] * (len(p["rows"]) - 1) for p in st)      # all scores 64: row 0 alone, the rest with it
    chain = parts("km_chain_c30")[0]
    assert len({m[0] for m in chain["moves"]}) >= 4 and max(m[0] for m in chain["moves"]) <= 14    # 13 rounds, min = 2 .. 14
    moved = [m[1] for m in chain["moves"]]
    assert len(moved) > len(set(moved))                                        # a row moves in more than one round
    assert parts("km_chain_c5")[0]["moves"] == [] and parts("km_chain_c5")[0]["varzahl"] > 0
    assert len(parts("km_large")[0]["rows"]) == 1100 > 1024
    below, at = parts("km_distance_below")[0], parts("km_distance_100")[0]
    assert below["pairs"] == [] and below["vars"] == []
    assert [(i, j) for i, j, _ in at["pairs"]] == [(2, 102)] and at["vars"] == [2, 102]


def test_five_slot_update():
    """RR:2658-2688 swap for swap.  The ORDER of the slots is the sequence of swaps (pinned below); the centroid is a vote of
    the five and does not see it.  As a set the list equals the first five by (score descending, j ascending) whenever at
    least five scores are positive -- checked exhaustively over every table of 6 and 7 scores in 1 .. 3, ties at the fifth
    place included -- and differs where fewer are: the initial (0, j = 0) slots survive and row 0 is counted again."""
    assert km.top5([5, 5, 5, 5, 5, 5, 9]) == [6, 3, 2, 1, 0]
    assert km.top5([4, 6, 6, 8, 6, 6, 6, 6, 7]) == [8, 4, 2, 1, 3]
    for n in (6, 7):
        for t in itertools.product((1, 2, 3), repeat=n):
            assert sorted(km.top5(list(t))) == sorted(sorted(range(n), key=lambda j: (-t[j], j))[:5])
    assert sorted(km.top5([7, 9, 8])) == [0, 0, 0, 1, 2]                       # three rows: row 0 three times
    table = [0, 0, 3, 0, 0, 0]
    assert sorted(km.top5(table)) == [0, 0, 0, 0, 2] != sorted(sorted(range(6), key=lambda j: (-table[j], j))[:5])


def test_host_chain_equals_the_checker():
    """pgr_kmeans_reassign (plain C) on the scores of km_chain_c30's part: 13 rounds, rows moving in several"""
    from repeatresolver_amd.kmeans_subdivision import reassign
    _lib()
    rec, first, case, win, ref, sub, got = checker_run("km_chain_c30")
    p = got["eligible"][0]
    I, Vars = p["rows"], p["vars"]
    sc_km = len(Vars) // 64 + 1
    vs = np.zeros((len(I), sc_km * 64), dtype=np.int64)
    for j, v in enumerate(Vars):
        vs[:, j] = win.G[v][I]
    own = km.match_matrix(vs, vs, sc_km).tolist()
    cent = np.zeros_like(vs)
    for i in range(len(I)):
        cent[i, :len(Vars)] = (vs[km.top5(own[i])].sum(axis=0) > 2)[:len(Vars)]
    scores = km.match_matrix(cent, vs, sc_km)
    assert list(reassign(scores, p["before"], case["cov"] // 2)) == p["after"] != p["before"]
    assert list(reassign(scores, p["before"], 2)) == p["before"]               # mingroup <= 2: no round


def test_no_eligible_part_needs_no_device():
    """bis_beyond has no part with more than 2 * mingroup rows: the compressed, completed input comes back; labels fed
    relabelled (3 x + 7) so that the compression has something to do"""
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide, last_timing
    from test_subdivision import as_refined
    _lib()
    rec, first, case, win, ref, sub, got = checker_run("bis_beyond")
    assert got["eligible"] == []
    lab = np.where(sub["reldrop_labels"] >= 0, sub["reldrop_labels"] * 3 + 7, -1)
    out = kmeans_subdivide(case["rows"], as_refined(ref), lab, case["von"], case["bis"], case["cov"])
    assert out.eligible == 0 and out.parts == out.parts_before == got["parts"]
    assert sd.subdivision_bytes(out.labels) == rec["kmeans"]["text"].encode()
    t = last_timing()
    assert t["pairs_ms"] == 0 and t["kmeans_ms"] == 0


def test_argument_errors():
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide
    from repeatresolver_amd.realigner import PwrError
    from test_subdivision import as_refined
    _lib()
    rec, first, case, win, ref, sub, got = checker_run("bis_beyond")
    assert (sub["reldrop_labels"] < 0).any()
    below = np.where(sub["reldrop_labels"] < 0, -5, sub["reldrop_labels"])   # a left-out row labelled below -1
    for bad_cov, lab in ((-1, sub["reldrop_labels"]), (case["cov"], np.where(sub["reldrop_labels"] >= 0, -1, -1)), (case["cov"], below)):
        with pytest.raises(PwrError) as e:
            kmeans_subdivide(case["rows"], as_refined(ref), lab, case["von"], case["bis"], bad_cov)
        assert e.value.code == -1


def test_cli_usage_and_missing_maxcorrs(tmp_path):
    _lib()
    p = subprocess.run([CLI], capture_output=True)
    assert p.returncode == 0 and p.stdout.decode().splitlines() == ["Usage: ./RepeatResolver MApath <options>"]      # RR:3869
    (tmp_path / "MSA").write_bytes(rc.msa_bytes(kc.case_input("km_distance_100")["rows"]))
    p = subprocess.run([CLI, "MSA", "-c", "10"], cwd=tmp_path, capture_output=True)
    assert p.returncode == 1 and "MaxCorrsOf_MSA is missing" in p.stdout.decode()
    assert not [n for n in os.listdir(tmp_path) if "SubdivisionOf_" in n]
