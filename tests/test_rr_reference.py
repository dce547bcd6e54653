"""Runs without a GPU: MaxCorrelation's restatement (oracle/mc_oracle.c), the checkers of the group refinement and the
subdivisions (tests/gr_checker.py, tests/sd_checker.py) and the host pieces of include/pgr.h against what the REFERENCE
wrote -- tests/golden/rr_reference.json.gz, recorded by oracle/gen_rr_fixtures.py from the unmodified MaxCorrelation.c and
RepeatResolver.c linked with the stand-in oracle/gsl_standin.c for their three GSL functions.  The stand-in itself is
compared with scipy here; its hypergeometric tail is the one tests/test_mc_oracle.py pins against exact rationals.  This is
not parity with a GSL-linked binary.

The inputs are regenerated from their seeds (tests/rr_cases.py); a test FAILS when the sha256 of its input is not the
fixture's.  The labels are compared byte for byte under the conditions of rr_cases.label_conditions, re-asserted here."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gr_checker as gc
import rr_cases as rc
import sd_checker as sd
from conftest import ROOT

LABEL_CASES = rc.fixture_names(labels=True)
ALL_CASES = rc.fixture_names()


def test_fixture_holds_the_cases_it_must():
    from test_gpu_group_refinement import CASES, fixture_cases
    from test_subdivision import REL_CASES
    assert set(CASES) | set(REL_CASES) | set(rc.RESEEDED) | {"stretched"} | {"realigned_" + n for n in fixture_cases()} <= set(LABEL_CASES)
    assert len(CASES) == 11 and len(REL_CASES) == 3 and len(fixture_cases()) >= 5
    assert {f"mc_{T}x{W}" for T, W in rc.MC_SHAPES} | {"mc_small_c4", "mc_small_c12", "mc_small_c30"} <= set(ALL_CASES)
    for name in ALL_CASES:
        rec = rc.load_fixture()[name]
        assert rec["maxcorrs"]["lines"] == rec["width"] * 5
        assert all(text != "0.000000" for _, text in rec["maxcorrs"]["nonzero"])
        assert rc.stdout_value(rec, "mc", "There are ") == f"There are {rec['rows']} sequences."
        assert rc.stdout_value(rec, "mc", "Siglength is ") == f"Siglength is {rec['width']}."


@functools.lru_cache(maxsize=None)
def checker_run(name):
    """(fixture record, case, the checker's window, refined arrays and subdivision) fed the REFERENCE's MaxCorrs values"""
    rec, case = rc.checked_input(name)
    win = gc.Window(case["rows"], rc.maxcorrs_values(rec), case["von"], case["bis"], case["cov"])
    ref = win.refine()
    return rec, case, win, ref, sd.subdivide(win, ref, case["cov"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_mc_oracle_against_the_reference_file(name):
    """zero pattern identical, values within 1.5e-6, at most 0.5 % of the "%f" lines different (the reference against the
    oracle gave 0 differing lines on the machine that made the fixture: the margin only covers another libm)"""
    rec, case = rc.checked_input(name)
    got = gc.mco_maxcorrs(case["rows"], case["cov"])
    differing = rc.compare_maxcorrs_text(["%f" % v for v in got], rc.maxcorrs_lines(rec))
    print(f"{name}: {differing} of {len(got)} lines differ")
    assert rc.stdout_value(rec, "mc", "Cutoff ") == "Cutoff %f" % (-1.0 * np.log10(1.0 / (rec["width"] * 5.0)))   # MC:998


@pytest.mark.parametrize("name", LABEL_CASES)
def test_conditions_of_the_exact_comparison(name):
    rec, case, win, ref, _ = checker_run(name)
    condition, sig, und = rc.label_conditions(case, rec, (win, ref))
    assert condition == rec["condition"] and (condition == "strict") == (und == [])
    assert (condition == "clique_sets") == (name in ("kept64", "kept65", "rel5groups")) and len(und) <= 1


@pytest.mark.parametrize("name", LABEL_CASES)
def test_checkers_against_the_reference_labels(name):
    rec, case, win, ref, got = checker_run(name)
    von, bis = case["von"], case["bis"]
    assert sd.subdivision_bytes(got["dropoff_labels"]) == rec["dropoff"]["text"].encode()
    assert sd.subdivision_bytes(got["reldrop_labels"]) == rec["reldrop"]["text"].encode()
    assert sd.subdivision_name("Dropoff", von, bis, rc.MSA_NAME) == rec["dropoff"]["file"]
    assert sd.subdivision_name("RelDrop", von, bis, rc.MSA_NAME) == rec["reldrop"]["file"]
    assert rc.stdout_value(rec, "rr", "Of ") == f"Of {len(case['rows'])} sequences, {win.T} had full coverage."
    assert rc.stdout_value(rec, "rr", "Siglength was ") == f"Siglength was {rec['width']} is now {win.w} from {win.von} to {win.bis}."
    mc = rc.maxcorrs_values(rec)[win.von * 5:(win.bis + 1) * 5]      # counted before the coverage restriction (RR:3981)
    assert [l for l in rec["stdout"]["rr"] if l.endswith("correlations make the cutoff.")] == [f"{int((mc > win.cutoff).sum())} correlations make the cutoff."]
    assert len(win.significant) <= int((mc > win.cutoff).sum())
    assert rc.stdout_value(rec, "rr", "Cutoff ") == "Cutoff %f" % win.cutoff
    assert rc.stdout_value(rec, "rr", "Maxcov: ") == f"Maxcov: {win.maxcov}"


def test_names_and_structure_of_the_special_cases():
    fx = rc.load_fixture()
    assert fx["bis_beyond"]["dropoff"]["file"] == "DropoffSubdivisionOf_60_5000_MSA" and fx["bis_beyond"]["reldrop"]["file"] == "RelDropSubdivisionOf_60_5000_MSA"
    assert fx["kept63"]["dropoff"]["file"] == "DropoffSubdivisionOf_0_1500000_MSA"
    assert fx["window"]["reldrop"]["file"] == "RelDropSubdivisionOf_120_330_MSA"
    # `stretched`: the only input on which the reference itself makes k_gr_reldrop walk more than one pass of 64 partitions
    rec, case, win, ref, got = checker_run("stretched")
    assert (rec["rows"], rec["width"], len(ref["significant"])) == (639, 1554, 142)
    assert (got["dropoff_parts"], got["reldrop_parts"]) == (192, 193) and [k for k, _, _ in got["splits"]] == [40]
    eligible = sum(int((got["dropoff_labels"] == k).sum()) > 2 * (case["cov"] // 2) for k in range(192))
    assert eligible > rc.KERNEL_TILE
    for name in ("rel8", "rel21", "rel5groups", "rel5groups_reseeded"):
        got = checker_run(name)[4]
        assert len(got["splits"]) == 1 and got["reldrop_parts"] == got["dropoff_parts"] + 1


def _lib():
    subprocess.run(["make", "-C", os.path.join(ROOT, "repeatresolver_amd", "csrc"), "all"], check=True, stdout=subprocess.DEVNULL)
    from repeatresolver_amd import _lib
    return _lib.load()


def read_maxcorrs_file(lib, path, von, bis):
    """pgr_read_maxcorrs_file through ctypes: the entries of columns von .. bis"""
    p, n = ctypes.c_void_p(), ctypes.c_int()
    assert lib.pgr_read_maxcorrs_file(str(path).encode(), von, bis, ctypes.byref(p), ctypes.byref(n)) == 0
    out = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), shape=(max(1, n.value),))[:n.value].copy()
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    libc.free(p)
    return out


@pytest.mark.parametrize("name", LABEL_CASES)
def test_host_pieces_against_the_reference(name, tmp_path):
    """include/pgr.h's plain C on the reference's data: the window reader, the MaxCorrs file reader on a file rebuilt from the
    fixture, the default cutoff and the coverage restriction, stage 1, the renumbering and completion helpers, the label
    writer and the name helper"""
    from repeatresolver_amd.group_refinement import read_window
    from repeatresolver_amd.subdivision import dropoff_subdivision, subdivision_name, write_subdivision
    from test_subdivision import as_refined
    lib = _lib()
    rec, case, win, ref, exp = checker_run(name)
    rows, von, bis, cov = case["rows"], case["von"], case["bis"], case["cov"]
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    drop_ref = np.array([int(v) for v in rec["dropoff"]["text"].split("\n")], dtype=np.int32)
    rel_ref = np.array([int(v) for v in rec["reldrop"]["text"].split("\n")], dtype=np.int32)
    # the window reader: the reference's own counts, and the rows it left out are the rows it labels -1
    kept, v, b, G, LC, cover = read_window(rows, von, bis)
    assert rc.stdout_value(rec, "rr", "Of ") == f"Of {len(rows)} sequences, {int(kept.sum())} had full coverage."
    assert rc.stdout_value(rec, "rr", "Siglength was ") == f"Siglength was {len(rows[0])} is now {b + 1 - v} from {v} to {b}."
    assert np.array_equal(kept, drop_ref >= 0) and np.array_equal(kept, rel_ref >= 0)
    # the file reader
    path = tmp_path / ("MaxCorrsOf_" + rc.MSA_NAME)
    path.write_text("".join(l + "\n" for l in rc.maxcorrs_lines(rec)))
    mc = read_maxcorrs_file(lib, path, v, b)
    assert np.array_equal(mc, rc.maxcorrs_values(rec)[v * 5:(b + 1) * 5])
    # the default cutoff, the count over it and the coverage restriction
    cutoff = lib.pgr_default_cutoff(0.0, b + 1 - v)
    assert rc.stdout_value(rec, "rr", "Cutoff ") == "Cutoff %f" % cutoff
    assert [l for l in rec["stdout"]["rr"] if l.endswith("make the cutoff.")] == [f"{int((mc > cutoff).sum())} correlations make the cutoff."]
    maxcov = ctypes.c_int()
    cover = np.ascontiguousarray(cover, dtype=np.int32)
    assert lib.pgr_restrict_coverage(b + 1 - v, cover.ctypes.data_as(pi), mc.ctypes.data_as(pd), ctypes.byref(maxcov)) == 0
    assert rc.stdout_value(rec, "rr", "Maxcov: ") == f"Maxcov: {maxcov.value}"
    assert np.array_equal(np.flatnonzero(mc > cutoff), ref["significant"])
    # stage 1 on the host from the checker's refined arrays (which the test above ties to the reference's labels)
    labels, parts = dropoff_subdivision(as_refined(ref), cov)
    assert parts == max(1, drop_ref.max() + 1)                        # no kept row: stage 1 still starts at one (empty) part
    full = np.zeros(len(rows), dtype=np.int32)
    k8 = kept.astype(np.uint8)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    assert lib.pgr_complete_labels(len(rows), k8.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), labels.ctypes.data_as(pi), full.ctypes.data_as(pi)) == 0
    assert np.array_equal(full, drop_ref)
    # the renumbering: the reference's kept labels are already renumbered by first appearance; a relabelling is undone
    for lab_ref in (drop_ref, rel_ref):
        lab = np.ascontiguousarray(lab_ref[kept] * 3 + 7, dtype=np.int32)
        assert lib.pgr_compress_labels(len(lab), lab.ctypes.data_as(pi)) == lab_ref.max() + 1 and np.array_equal(lab, lab_ref[kept])
    # the writer and the names
    for stage, lab_ref, want in (("Dropoff", drop_ref, rec["dropoff"]), ("RelDrop", rel_ref, rec["reldrop"])):
        fname = subdivision_name(stage, von, bis, rc.MSA_NAME)
        assert fname == want["file"]
        write_subdivision(tmp_path / fname, lab_ref)
        assert (tmp_path / fname).read_bytes() == want["text"].encode()


@pytest.fixture(scope="module")
def standin():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libgslstandin.so"))
    for n in ("gsl_cdf_hypergeometric_Q", "gsl_cdf_hypergeometric_P"):
        getattr(lib, n).restype = ctypes.c_double
        getattr(lib, n).argtypes = [ctypes.c_uint] * 4
    lib.gsl_cdf_binomial_Q.restype = ctypes.c_double
    lib.gsl_cdf_binomial_Q.argtypes = [ctypes.c_uint, ctypes.c_double, ctypes.c_uint]
    return lib


def test_standin_against_scipy(standin):
    """the ranges and the tolerance of test_hypergeometric_tail_against_scipy (tests/test_mc_oracle.py): P against
    hypergeom.cdf, Q is the pinned tail itself (the same function, not a copy), the binomial against binom.sf"""
    from fractions import Fraction
    from math import comb
    from scipy.stats import binom, hypergeom
    mco = gc.mco()
    rng = np.random.default_rng(1)
    hyp = []
    for _ in range(4000):
        n1 = int(rng.integers(1, 600)); n2 = int(rng.integers(0, 600)); t = int(rng.integers(1, n1 + n2 + 1)); k = int(rng.integers(0, min(n1, t) + 1))
        hyp.append((k, n1, n2, t))
    k, n1, n2, t = np.array(hyp).T
    for (k_, n1_, n2_, t_), cdf, sf in zip(hyp, hypergeom.cdf(k, n1 + n2, n1, t), hypergeom.sf(k, n1 + n2, n1, t)):   # scipy once, on arrays
        p = standin.gsl_cdf_hypergeometric_P(k_, n1_, n2_, t_)
        assert p == pytest.approx(cdf, rel=1e-10, abs=1e-300), (k_, n1_, n2_, t_)
        q = standin.gsl_cdf_hypergeometric_Q(k_, n1_, n2_, t_)
        assert q == mco.mco_hyper_Q(k_, n1_, n2_, t_)
        assert q == pytest.approx(sf, rel=1e-10, abs=1e-300), (k_, n1_, n2_, t_)
    bino = [(int(rng.integers(0, n + 1)), float(rng.random()), n) for n in (int(rng.integers(1, 600)) for _ in range(4000))]
    k, pr, n = (np.array(x) for x in zip(*bino))
    tiny = 0
    for (k_, pr_, n_), ref in zip(bino, binom.sf(k, n, pr)):
        q = standin.gsl_cdf_binomial_Q(k_, pr_, n_)
        if ref < 1e-250 and k_ < n_:
            # scipy's own intermediates underflow down here (it returns 0.0 for tails near 1e-295): the exact rational decides
            a, b = pr_.as_integer_ratio()                             # pr_ = a / b exactly
            ref = float(Fraction(sum(comb(n_, i) * a ** i * (b - a) ** (n_ - i) for i in range(k_ + 1, n_ + 1)), b ** n_))
            tiny += 1
        assert q == pytest.approx(ref, rel=1e-10, abs=1e-300), (k_, pr_, n_)
    assert tiny < 400
    # the arguments BestCutoff gives it (RR:1659: p = 0.70 and 0.05, v = Sizes up to 30), and the edges
    for v in range(1, 31):
        for c in range(v):
            for pr in (0.70, 0.05):
                assert standin.gsl_cdf_binomial_Q(c, pr, v) == pytest.approx(binom.sf(c, v, pr), rel=1e-10, abs=1e-300)
    assert standin.gsl_cdf_binomial_Q(5, 0.3, 5) == 0.0 and standin.gsl_cdf_binomial_Q(0, 0.0, 5) == 0.0 and standin.gsl_cdf_binomial_Q(2, 1.0, 5) == 1.0
    assert standin.gsl_cdf_hypergeometric_P(7, 7, 9, 12) == 1.0 and standin.gsl_cdf_hypergeometric_Q(7, 7, 9, 12) == 0.0
