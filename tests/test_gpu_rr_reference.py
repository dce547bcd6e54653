"""-m gpu: the HIP MaxCorrelation (include/pmc.h), the group refinement (k_gr_cliques, k_gr_votes) and the drop-off
subdivisions (k_gr_reldrop) of include/pgr.h against what the REFERENCE wrote: tests/golden/rr_reference.json.gz, recorded
by oracle/gen_rr_fixtures.py from the unmodified MaxCorrelation.c and RepeatResolver.c linked with a stand-in for their
three GSL functions (oracle/gsl_standin.c; not a GSL-linked binary).  Nothing here reads the reference or a binary made
from it; the inputs are regenerated from their seeds and a test FAILS when the sha256 of its input is not the fixture's.

MaxCorrsOf_ files are compared by the three criteria of test_cli_writes_the_reference_file (zero pattern identical, values
within 1.5e-6, at most 0.5 % of the "%f" lines different).  Label files are compared byte for byte; tests/test_rr_reference.py
asserts on the CPU the conditions that make that legitimate (rr_cases.label_conditions)."""
import numpy as np
import pytest

import rr_cases as rc
from test_rr_reference import read_maxcorrs_file

pytestmark = pytest.mark.gpu

LABEL_CASES = rc.fixture_names(labels=True)
END_TO_END = ["stretched", "stretched_deep", "rel8", "rel21", "rel5groups", "rel5groups_reseeded"]


def write_msa(tmp_path, case):
    (tmp_path / rc.MSA_NAME).write_bytes(rc.msa_bytes(case["rows"]))


def device_maxcorrs_file(tmp_path, rec, case):
    """the drop-in binary on the MSA in tmp_path: its MaxCorrsOf_ lines, after the comparison with the reference's"""
    from repeatresolver_amd.max_correlation import run_file
    code, lines = run_file(rc.MSA_NAME, mincov=case["cov"], cwd=str(tmp_path))
    assert code == 0, lines
    assert rc.stdout_value(rec, "mc", "There are ") in lines and rc.stdout_value(rec, "mc", "Siglength is ") in lines
    text = (tmp_path / ("MaxCorrsOf_" + rc.MSA_NAME)).read_text()
    assert text.endswith("\n")
    got = text.split("\n")[:-1]
    differing = rc.compare_maxcorrs_text(got, rc.maxcorrs_lines(rec))
    print(f"{rec['name']}: {differing} of {len(got)} '%f' lines differ between device and reference")
    return got


def chain_and_compare(tmp_path, rec, case):
    """tmp_path/MaxCorrsOf_MSA through the product's file reader, refine_groups, the device subdivision and the product's
    writer: both files byte-equal to the reference's, under the reference's names"""
    from repeatresolver_amd import _lib
    from repeatresolver_amd.group_refinement import refine_groups
    from repeatresolver_amd.subdivision import subdivide, subdivision_name, write_subdivision
    rows, von, bis, cov = case["rows"], case["von"], case["bis"], case["cov"]
    full = read_maxcorrs_file(_lib.load(), tmp_path / ("MaxCorrsOf_" + rc.MSA_NAME), 0, len(rows[0]) - 1)
    assert len(full) == len(rows[0]) * 5
    refined = refine_groups(rows, full, von, bis, cov)
    got = subdivide(rows, refined, von, bis, cov)
    for stage, labels, want in (("Dropoff", got.dropoff_labels, rec["dropoff"]), ("RelDrop", got.reldrop_labels, rec["reldrop"])):
        name = subdivision_name(stage, von, bis, rc.MSA_NAME)
        assert name == want["file"]
        write_subdivision(tmp_path / name, labels)
        data = (tmp_path / name).read_bytes()
        if data != want["text"].encode():
            a, b = np.array(labels), np.array([int(v) for v in want["text"].split("\n")])
            raise AssertionError(f"{rec['name']} {stage}: {int((a != b).sum()) if a.shape == b.shape else 'all'} of {len(b)} labels differ "
                                 f"({got.dropoff_parts} -> {got.reldrop_parts} parts, {got.eligible} eligible, {got.selected} selected)")
    return got


@pytest.mark.parametrize("name", rc.fixture_names())
def test_device_maxcorrelation_against_the_reference_file(name, tmp_path):
    rec, case = rc.checked_input(name)
    write_msa(tmp_path, case)
    device_maxcorrs_file(tmp_path, rec, case)


@pytest.mark.parametrize("name", LABEL_CASES)
def test_chain_from_the_reference_maxcorrs(name, tmp_path):
    """refinement and subdivision on the device from the REFERENCE's MaxCorrs values"""
    rec, case = rc.checked_input(name)
    (tmp_path / ("MaxCorrsOf_" + rc.MSA_NAME)).write_text("".join(l + "\n" for l in rc.maxcorrs_lines(rec)))
    got = chain_and_compare(tmp_path, rec, case)
    if name.startswith("stretched"):
        assert got.dropoff_parts == 192 and got.eligible > rc.KERNEL_TILE          # more than one pass of k_gr_reldrop
        split = np.flatnonzero(got.winner >= 0)
        assert got.reldrop_parts == 192 + len(split) and len(split) >= 1
        assert (split >= rc.KERNEL_TILE).all() if name == "stretched_deep" else list(split) == [40]


@pytest.mark.parametrize("name", END_TO_END)
def test_chain_end_to_end(name, tmp_path):
    """device MaxCorrelation, its file written and read again at six decimals, refinement, subdivision: the reference's labels"""
    rec, case = rc.checked_input(name)
    write_msa(tmp_path, case)
    device_maxcorrs_file(tmp_path, rec, case)
    chain_and_compare(tmp_path, rec, case)
