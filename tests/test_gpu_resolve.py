"""-m gpu: pgr_msa_resolve (include/pgr.h) -- every window read by the device reader, refined on the sets it left on the
device, subdivided and clustered -- against (a) the chain of the literal checkers gr_checker / sd_checker / km_checker fed the
same MaxCorrs and (b) the per-window path (pipeline.clustered; refine_groups, subdivide, kmeans_subdivide), which the
existing fixtures pin to the reference.  Labels and part counts are integers and compared exactly; the conditions of that
exact comparison are re-asserted here (no undecided variation, no MaxCorrs value within 1e-5 of the cutoff, no k-means pair
within 1e-8 of it): conditions, not skips.  connect on the labels against tests/cn_checker.py at 1e-10 (derivation:
tests/test_connect.py).  The drop-in's -w against its own -f runs, byte for byte.

Main input: ragged(31), 240 rows x 900 columns, four planted copy groups of 40 distinguishing columns, two rows of three
blank at scattered ends; sites 100, 350, 600, 850; cov 12.  Checked on the CPU with the oracle's MaxCorrs: 108 / 144 / 96 kept
rows, 4 parts after every stage in every window, 4 eligible parts per window (every kernel runs), 97 and 92 rows shared by
neighbouring windows."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import cn_checker as cn
import gr_checker as gc
import km_checker as km
import sd_checker as sd
from conftest import ROOT
from test_gpu_group_refinement import checked, planted_msa

CSRC = os.path.join(ROOT, "repeatresolver_amd", "csrc")
CLI, MC_CLI = os.path.join(CSRC, "RepeatResolver"), os.path.join(CSRC, "MaxCorrelation")
SITES, COV = [100, 350, 600, 850], 12


@functools.lru_cache(maxsize=None)
def ragged(seed=31, T=240, W=900, closed=False):
    base = planted_msa(seed, T, W, [40, 40, 40, 40], extra=0, inner_blanks=False)
    rng = np.random.default_rng(seed)
    rows = []
    for r, line in enumerate(base):
        row = bytearray(line)
        a, b = int(rng.integers(0, 500)), int(W - rng.integers(0, 500))
        if r % 3 == 0:
            a, b = 0, W
        row[:a] = b" " * a
        row[b:] = b" " * (W - b)
        if closed:
            row[W - 1:] = b" "
        rows.append(bytes(row))
    return rows


@functools.lru_cache(maxsize=None)
def checker_chain(closed=False):
    """(rows, the oracle's MaxCorrs, per window of SITES: the three checkers' results and the conditions); once per process"""
    rows = ragged(closed=closed)
    mc = gc.mco_maxcorrs(rows, COV)
    out = []
    for von, bis in zip(SITES[:-1], SITES[1:]):
        win = gc.Window(rows, mc, von, bis, COV)
        ref = win.refine()
        sub = sd.subdivide(win, ref, COV)
        kmr = km.clustered(win, ref, sub["reldrop_labels"], COV)
        und = [s for s in range(len(ref["significant"])) if gc.undecided(ref["candidates"][s], ref["cutoff"])]
        sliced = mc[von * 5:(bis + 1) * 5]
        nz = sliced[sliced != 0]
        out.append({"ref": ref, "sub": sub, "km": kmr, "undecided": len(und), "near": float(np.abs(nz - ref["cutoff"]).min()),
                    "margin": km.margin(kmr["eligible"], ref["cutoff"])})
    return rows, mc, out


@functools.lru_cache(maxsize=None)
def resolved_main():
    from repeatresolver_amd.resolution import open_msa, resolve
    rows, mc, _ = checker_chain()
    with open_msa(rows) as msa:
        return resolve(msa, mc, SITES, COV)


def per_window(rows, mc, von, bis, cov):
    """the entry points of one window, one after the other, on the same MaxCorrs"""
    from repeatresolver_amd.group_refinement import refine_groups
    from repeatresolver_amd.kmeans_subdivision import kmeans_subdivide
    from repeatresolver_amd.subdivision import subdivide
    refined = refine_groups(rows, mc, von, bis, cov)
    sub = subdivide(rows, refined, von, bis, cov)
    return refined, sub, kmeans_subdivide(rows, refined, sub, von, bis, cov)


def same_as_per_window(w, refined, sub, kms):
    assert w.kept_rows == int(refined.kept.sum()) and w.cutoff == refined.cutoff
    assert np.array_equal(w.dropoff_labels, sub.dropoff_labels) and np.array_equal(w.reldrop_labels, sub.reldrop_labels)
    assert np.array_equal(w.kmeans_labels, kms.labels)
    assert (w.dropoff_parts, w.reldrop_parts, w.kmeans_parts) == (sub.dropoff_parts, sub.reldrop_parts, kms.parts)


def test_input_and_conditions():
    """no GPU: the input is the one the numbers above were checked on, and the conditions of the exact comparisons hold"""
    rows, mc, chain = checker_chain()
    assert hashlib.sha256(b"\n".join(rows)).hexdigest().startswith("8fa8df5691019d61")
    assert [int(c["ref"]["kept"].sum()) for c in chain] == [108, 144, 96]
    for c in chain:
        assert (c["sub"]["dropoff_parts"], c["sub"]["reldrop_parts"], c["km"]["parts"]) == (4, 4, 4)
        assert len(c["km"]["eligible"]) == 4 and len(c["ref"]["significant"]) > 16 and c["sub"]["selected"] > 0
        assert c["undecided"] == 0 and c["near"] > 1e-5 and c["margin"] > 1e-8
    shared = [int(((a["km"]["labels"] > -1) & (b["km"]["labels"] > -1)).sum()) for a, b in zip(chain[:-1], chain[1:])]
    assert shared == [97, 92]


@pytest.mark.gpu
def test_labels_equal_the_checker_chain():
    _, _, chain = checker_chain()
    got = resolved_main()
    assert [(w.von, w.bis) for w in got] == list(zip(SITES[:-1], SITES[1:]))
    for w, c in zip(got, chain):
        assert w.kept_rows == int(c["ref"]["kept"].sum()) and w.cutoff == c["ref"]["cutoff"]
        assert np.array_equal(w.dropoff_labels, c["sub"]["dropoff_labels"])
        assert np.array_equal(w.reldrop_labels, c["sub"]["reldrop_labels"])
        assert np.array_equal(w.kmeans_labels, c["km"]["labels"])
        assert (w.dropoff_parts, w.reldrop_parts, w.kmeans_parts) == (c["sub"]["dropoff_parts"], c["sub"]["reldrop_parts"], c["km"]["parts"])


@pytest.mark.gpu
def test_labels_equal_the_per_window_path():
    """pipeline.clustered per window (its own MaxCorrelation on the device: within rounding of the oracle's, and no value is
    within 1e-5 of the cutoff), and the three entry points on the very same MaxCorrs"""
    from repeatresolver_amd.pipeline import clustered
    from repeatresolver_amd.resolution import last_timing
    rows, mc, _ = checker_chain()
    got = resolved_main()
    for w in got:
        sub, kms = clustered(rows, w.von, w.bis, COV)
        assert np.array_equal(w.dropoff_labels, sub.dropoff_labels) and np.array_equal(w.reldrop_labels, sub.reldrop_labels)
        assert np.array_equal(w.kmeans_labels, kms.labels)
        assert (w.dropoff_parts, w.reldrop_parts, w.kmeans_parts) == (sub.dropoff_parts, sub.reldrop_parts, kms.parts)
        same_as_per_window(w, *per_window(rows, mc, w.von, w.bis, COV))
    t = last_timing()
    assert t["upload_ms"] > 0 and t["reader_ms"] > 0 and t["refine_ms"] > 0 and t["subdivide_ms"] > 0 and t["kmeans_ms"] > 0
    assert t["resolve_ms"] >= t["reader_ms"] + t["refine_ms"] + t["subdivide_ms"] + t["kmeans_ms"]


@pytest.mark.gpu
def test_one_window_call():
    """the case `window` of tests/test_gpu_group_refinement.py as a one-window call"""
    from repeatresolver_amd.resolution import open_msa, resolve
    rows, mc, von, bis, cov, _ = checked("window")
    with open_msa(rows) as msa:
        got = resolve(msa, mc, [von, bis], cov)
    assert len(got) == 1 and 12 < got[0].kept_rows < len(rows)
    same_as_per_window(got[0], *per_window(rows, mc, von, bis, cov))


def outcome(call):
    from repeatresolver_amd.realigner import PwrError
    try:
        return 0, call()
    except PwrError as e:
        return e.code, None


@pytest.mark.gpu
def test_a_window_without_rows_and_a_window_outside():
    """A last window that keeps no row at all.  In ragged(31) every third row spans the whole width, so no window inside it
    is empty; here its last column is blanked in every row and a fourth site set on it: [850, 899] keeps nothing.  And a site
    beyond the width: the window starts behind the last column.  Outcome and return code are the per-window path's."""
    from repeatresolver_amd.resolution import open_msa, resolve
    rows = ragged(closed=True)
    mc = gc.mco_maxcorrs(rows, COV)
    sites = SITES + [899]
    exp_code, exp = outcome(lambda: [per_window(rows, mc, a, b, COV) for a, b in zip(sites[:-1], sites[1:])])
    with open_msa(rows) as msa:
        code, got = outcome(lambda: resolve(msa, mc, sites, COV))
        assert code == exp_code
        if exp_code == 0:
            assert got[-1].kept_rows == 0 and (got[-1].kmeans_labels == -1).all() and got[0].kept_rows == 108
            for w, e in zip(got, exp):
                same_as_per_window(w, *e)
        outside = [100, 350, 900, 950]
        exp_code, _ = outcome(lambda: [per_window(rows, mc, a, b, COV) for a, b in zip(outside[:-1], outside[1:])])
        assert exp_code == -1 and outcome(lambda: resolve(msa, mc, outside, COV))[0] == -1
        for bad in ([100], [100, 100], [350, 100], [-1, 100], []):
            assert outcome(lambda: resolve(msa, mc, bad, COV))[0] == -1


@pytest.mark.gpu
def test_connect_on_the_resolved_labels():
    from repeatresolver_amd.resolution import connect
    labels = [w.kmeans_labels for w in resolved_main()]
    got = connect(labels)
    exp = cn.connection_matrix([l.tolist() for l in labels])
    assert got.matrix.shape == (4, 4) and np.abs(got.matrix - exp).max() <= 1e-10
    assert cn.decided(exp)
    best, conf, mutual = cn.best_columns(exp)
    assert np.array_equal(got.best, best) and np.array_equal(got.mutual, mutual) and np.abs(got.confidence - conf).max() <= 1e-10
    assert sorted(got.best.tolist()) == [0, 1, 2, 3] and got.mutual.all()     # the planted copies are found across the windows


@pytest.mark.gpu
def test_pipeline_resolved():
    """pipeline.resolved with parts=3 equals the same chain called piece by piece"""
    from repeatresolver_amd.max_correlation import max_correlations
    from repeatresolver_amd.pipeline import resolved
    from repeatresolver_amd.resolution import connect, open_msa, resolve
    from repeatresolver_amd.window import window_boundaries
    rows = ragged()
    sites, windows, con = resolved(rows, parts=3, cov=COV)
    assert sites == window_boundaries(rows, 0.90, 3) and len(windows) == 3
    mc = max_correlations(rows, COV)
    with open_msa(rows) as msa:
        exp = resolve(msa, mc, sites, COV)
    for w, e in zip(windows, exp):
        assert (w.von, w.bis, w.kept_rows, w.kmeans_parts) == (e.von, e.bis, e.kept_rows, e.kmeans_parts)
        assert np.array_equal(w.dropoff_labels, e.dropoff_labels) and np.array_equal(w.reldrop_labels, e.reldrop_labels)
        assert np.array_equal(w.kmeans_labels, e.kmeans_labels)
    assert np.array_equal(con.matrix, connect([e.kmeans_labels for e in exp]).matrix)


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=120)


def write_inputs(d, with_maxcorrs):
    import ctypes
    from repeatresolver_amd import _lib
    rows, mc, _ = checker_chain()
    d.mkdir()
    (d / "MSA").write_bytes(b"\n".join(rows) + b"\n")
    if with_maxcorrs:
        rc = _lib.load().pmc_write(str(d / "MaxCorrsOf_MSA").encode(), len(mc), mc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert rc == 0


def label_files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d)) if "SubdivisionOf_" in n}


@pytest.mark.gpu
def test_cli_w_equals_the_f_runs(tmp_path):
    from repeatresolver_amd.resolution import connect
    one, each = tmp_path / "one", tmp_path / "each"
    write_inputs(one, True)
    write_inputs(each, True)
    p = run([CLI, "MSA", "-c", str(COV), "-w"] + [str(s) for s in SITES], one)
    assert p.returncode == 0, p.stdout + p.stderr
    lines_f = []
    for a, b in zip(SITES[:-1], SITES[1:]):
        q = run([CLI, "MSA", "-c", str(COV), "-f", str(a), str(b)], each)
        assert q.returncode == 0, q.stdout + q.stderr
        lines_f += [l for l in q.stdout.splitlines() if l.startswith(("Full coverage", "Cutoff", "Parts"))]
    got, exp = label_files(one), label_files(each)
    assert len(exp) == 9 and got == exp
    assert [l for l in p.stdout.splitlines() if l.startswith(("Full coverage", "Cutoff", "Parts"))] == lines_f
    text = (one / "ConnectionsOf_100_850_MSA").read_text().splitlines()
    labels = [np.array(exp[f"KmeansSubdivisionOf_{a}_{b}_MSA"].split(), dtype=np.int32) for a, b in zip(SITES[:-1], SITES[1:])]
    con = connect(labels)
    assert text[0].split() == [str(con.matrix.shape[0]), str(con.matrix.shape[1])] and len(text) == 1 + con.matrix.shape[0]
    parsed = np.array([[float(v) for v in l.split(" ")] for l in text[1:]])
    assert parsed.shape == con.matrix.shape and np.abs(parsed - con.matrix).max() <= 5e-7
    assert not (each / "ConnectionsOf_100_850_MSA").exists()


@pytest.mark.gpu
def test_cli_w_computes_a_missing_maxcorrs_file(tmp_path):
    with_file, without, mcdir = tmp_path / "with", tmp_path / "without", tmp_path / "mc"
    write_inputs(with_file, True)
    write_inputs(without, False)
    write_inputs(mcdir, False)
    args = [CLI, "MSA", "-c", str(COV), "-w"] + [str(s) for s in SITES]
    q = run([CLI, "MSA", "-c", str(COV), "-f", "100", "350"], without)
    assert q.returncode == 1 and not label_files(without) and not (without / "MaxCorrsOf_MSA").exists()
    assert run(args, with_file).returncode == 0
    p = run(args, without)
    assert p.returncode == 0, p.stdout + p.stderr
    m = run([MC_CLI, "MSA", "-c", str(COV)], mcdir)
    assert m.returncode == 0, m.stdout + m.stderr
    assert (without / "MaxCorrsOf_MSA").read_bytes() == (mcdir / "MaxCorrsOf_MSA").read_bytes()
    assert len(label_files(without)) == 9 and label_files(without) == label_files(with_file)
