"""-m gpu: pgr_msa_consensus (include/pgr.h; k_cs_counts, k_cs_consensus, k_cs_diff of pgr_cons_device.hip) through
resolution.consensus against tests/ta_checker.py, the plain restatement of TransposonAssessment.py's GroupMaker, Konsensus,
SignaturesMaker and Diff.  Counts, consensus, depth, selected columns and both diff matrices are integers and compared exactly;
there is no tolerance in this file.  The conditions of the main input (ragged(31) of tests/test_gpu_resolve.py, cutoff 10.0: no
column within 0.3 of the cutoff, no tied column in any window's k-means parts) are asserted without a GPU in
tests/test_consensus.py.

Shapes: the kernel's constants are cs_cases.KERNEL_TILE = 1024 window columns and KERNEL_ROWS = 255 rows of a part per
work-group (its counters have 8 bits), four columns per thread, a wave per pair of parts in k_cs_diff, and KERNEL_SCRATCH_INTS count entries per range of
columns.  So: windows narrower than a tile (the main input), 1027 columns = one tile and three columns of a second, parts of
2R + 1, R and 1 rows (atomics, plain stores, and columns where all R rows agree: a counter at 255), an odd row stride with von = 3 (every byte alignment of a row's first word), a one-column window, a
window ending in the last column of the last row (the last word of the text), 130 parts (8385 pairs), and 640 parts x 11000
columns x 5 = 35.2 M count entries, which is two ranges of columns."""
import functools

import numpy as np
import pytest

import cs_cases as cs
import ta_checker as ta
from test_gpu_resolve import COV, SITES, checker_chain, ragged


def by_hand(rows, labels, von=None, bis=None, maxcorrs=None, cutoff=1.0, counts=True):
    from repeatresolver_amd.resolution import consensus, open_msa
    with open_msa(rows) as msa:
        return consensus(msa, labels, von, bis, maxcorrs, cutoff, counts=counts)


@pytest.mark.gpu
def test_the_hand_made_case():
    con = by_hand(cs.HAND_ROWS, cs.HAND_LABELS, maxcorrs=cs.hand_maxcorrs())
    cs.same(con, ta.consensus(cs.HAND_ROWS, cs.HAND_LABELS, None, None, cs.hand_maxcorrs(), 1.0))
    assert con.consensus.tolist() == cs.HAND_CONSENSUS and con.depth.tolist() == cs.HAND_DEPTH
    assert con.selected.tolist() == cs.HAND_SELECTED and con.diff[0, 1] == cs.HAND_DIFF and con.diff_all[0, 1] == cs.HAND_DIFF_ALL
    assert con.sequences() == cs.HAND_SEQUENCES and con.part_label.tolist() == [0, 2] and con.part_rows.tolist() == [2, 3]
    sub = by_hand(cs.HAND_ROWS, cs.HAND_LABELS, 2, 6, counts=False)
    assert sub.counts is None
    cs.same(sub, ta.consensus(cs.HAND_ROWS, cs.HAND_LABELS, 2, 6), counts=False)


@pytest.mark.gpu
def test_the_windows_of_the_main_input():
    """every window of SITES with the checker chain's k-means labels, the oracle's MaxCorrs and cutoff 10.0"""
    from repeatresolver_amd.resolution import consensus, last_consensus_timing, open_msa
    rows, mc, chain = checker_chain()
    with open_msa(rows) as msa:
        for (von, bis), c in zip(zip(SITES[:-1], SITES[1:]), chain):
            labels = c["km"]["labels"]
            con = consensus(msa, labels, von, bis, mc, cs.CUTOFF, counts=True)
            cs.same(con, ta.consensus(rows, labels, von, bis, mc, cs.CUTOFF))
            assert con.parts == 4 and con.diff.min() == 0 and con.diff[~np.eye(4, dtype=bool)].min() > 0
        t = last_consensus_timing()
        assert t["counts_ms"] > 0 and t["consensus_diff_ms"] > 0 and t["all_ms"] >= t["counts_ms"] + t["consensus_diff_ms"] + t["download_ms"]


@pytest.mark.gpu
def test_the_whole_width_of_the_main_input():
    """von = bis = None and a labelling of all rows: the rows blank at their ends give varying depth"""
    rows, mc, _ = checker_chain()
    labels = np.arange(len(rows), dtype=np.int32) % 7
    exp = ta.consensus(rows, labels, None, None, mc, cs.CUTOFF)
    assert len(set(exp["depth"][0].tolist())) > 5 and len(exp["selected"]) == 160
    cs.same(by_hand(rows, labels, None, None, mc, cs.CUTOFF), exp)


@functools.lru_cache(maxsize=None)
def geometry():
    text, mc = cs.random_msa(1, 900, 1031)
    text = text.copy()
    text[:, 100:108] = np.frombuffer(b"aAcgT-_a", dtype=np.uint8)      # columns where every row of a part agrees: counts of R and 2R + 1
    return [r.tobytes() for r in text], text, mc, cs.geometry_labels(900)


@pytest.mark.gpu
@pytest.mark.parametrize("von,bis", [(3, 1029), (517, 517), (1030, 1030), (0, 1030), (998, 1030), (2, 1025)])
def test_geometry(von, bis):
    """900 x 1031 over the full alphabet, a quarter blank: parts of 2R + 1, R and 1 rows and rows at -1; [3, 1029] is 1027
    columns, no multiple of the tile; one-column windows; windows ending in the last column; [2, 1025] is one tile exactly"""
    from repeatresolver_amd.resolution import consensus, open_msa
    rows, text, mc, labels = geometry()
    assert sorted(np.bincount(labels[labels >= 0]).tolist())[-3:] == [1, cs.KERNEL_ROWS, 2 * cs.KERNEL_ROWS + 1] and (labels == -1).sum() > 100
    assert (bis + 1 - von) % cs.KERNEL_TILE != 0 or (von, bis) == (2, 1025)
    exp = ta.consensus(rows, labels, von, bis, mc, 1.0)
    with open_msa(text) as msa:
        con = consensus(msa, labels, von, bis, mc, 1.0, counts=True)
    cs.same(con, exp)
    assert con.part_label.tolist() == [1, 4, 9]
    if bis - von > 1000:
        assert exp["counts"].max() == 2 * cs.KERNEL_ROWS + 1 and (exp["counts"] == cs.KERNEL_ROWS).sum() >= 8
    if bis - von > 100:
        assert (exp["depth"] == 0).any() and ta.tied_columns(exp["counts"]) > 0 and 0 < len(exp["selected"]) < bis + 1 - von


@pytest.mark.gpu
def test_many_parts():
    """130 parts of one to five rows: 8385 pairs, more than the 64 x 4 of one work-group row of k_cs_diff"""
    text, mc = cs.random_msa(3, 420, 301)
    rows = [r.tobytes() for r in text]
    labels = cs.many_parts_labels(420, 130)
    exp = ta.consensus(rows, labels, 1, 299, mc, 1.0)
    assert len(exp["part_label"]) == 130 and sorted(set(exp["part_rows"].tolist())) == [1, 2, 3, 4, 5]
    con = by_hand(text, labels, 1, 299, mc, 1.0)
    cs.same(con, exp)
    assert np.array_equal(con.diff, con.diff.T) and (np.diag(con.diff_all) == 0).all()


@pytest.mark.gpu
def test_column_ranges():
    """640 parts x 11000 columns x 5 exceeds KERNEL_SCRATCH_INTS: the window goes through in two ranges of whole tiles (10240
    and 760 columns), the diff matrices add up over them.  Against cs_cases.numpy_consensus, which tests/test_consensus.py
    compares with the checker."""
    parts, W = 640, 11000
    per_range = cs.KERNEL_SCRATCH_INTS // (parts * 5 * cs.KERNEL_TILE) * cs.KERNEL_TILE
    assert 0 < per_range < W <= 2 * per_range and per_range == 10240
    text, _ = cs.random_msa(4, 700, W + 3)
    rng = np.random.default_rng(6)
    labels = np.where(np.arange(700) < 660, np.arange(700) % parts, -1).astype(np.int32)[rng.permutation(700)]
    con = by_hand(text, labels, 2, W + 1, counts=False)
    kon, depth, d_all = cs.numpy_consensus(text, labels, 2, W + 1)
    assert con.parts == parts and con.consensus.shape == (parts, W)
    assert np.array_equal(con.consensus, kon) and np.array_equal(con.depth, depth)
    assert np.array_equal(con.diff_all, d_all) and np.array_equal(con.diff, d_all) and len(con.selected) == W


def code_of(call):
    from repeatresolver_amd.realigner import PwrError
    try:
        call()
        return 0
    except PwrError as e:
        return e.code


@pytest.mark.gpu
def test_errors_and_resolvability():
    from repeatresolver_amd import _lib
    from repeatresolver_amd.resolution import consensus, open_msa, resolvability
    rows, mc, chain = checker_chain()
    T, W = len(rows), len(rows[0])
    good = np.arange(T, dtype=np.int32) % 3
    with open_msa(rows) as msa:
        low = good.copy()
        low[5] = -2
        high = good.copy()
        high[7] = _lib.PGR_MAX_ROWS
        top = good.copy()
        top[7] = _lib.PGR_MAX_ROWS - 1                                 # the largest label there is: one more part
        for labels, von, bis, code in ((low, 0, 10, -1), (good, 10, 9, -1), (good, 0, W, -1), (good, -1, 5, -1), (good, W, W, -1),
                                       (np.full(T, -1), 0, 10, -1), ([None] * T, 0, 10, -1), (high, 0, 10, -5), (top, 0, 10, 0),
                                       (good, W - 1, W - 1, 0)):
            assert code_of(lambda: consensus(msa, labels, von, bis)) == code, (von, bis, code)
        assert consensus(msa, top, 0, 10).part_label.tolist() == [0, 1, 2, _lib.PGR_MAX_ROWS - 1]
        with pytest.raises(ValueError):
            consensus(msa, good[:-1], 0, 10)
        with pytest.raises(ValueError):
            consensus(msa, good, 0, None)
        with pytest.raises(ValueError):
            consensus(msa, good, 0, 10, mc[:-5])
        # resolvability with the script's start / ende (variation indices) against the checker, on the first window's k-means
        # labels as the truth; cutoff 10.0, where the main input's conditions hold
        truth = chain[0]["km"]["labels"]
        start, ende = 5 * SITES[0] + 3, 5 * SITES[1] + 4
        von, bis = ta.window_of(start, ende)
        assert (von, bis) == (SITES[0], SITES[1] - 1)
        exp = ta.consensus(rows, truth, von, bis, mc, cs.CUTOFF)
        summe, smallest, returned = ta.resolvability(exp["diff"].tolist())
        unique, parts, mind, last = resolvability(msa, truth, mc, start, ende, cs.CUTOFF)
        assert (unique, parts, mind.tolist(), last.tolist()) == (summe, 4, smallest, returned) and unique[0] == 4 and unique[10] == 4
        for start, ende in ((500, 504), (504, 500), (-5, 20)):
            with pytest.raises(ValueError):
                resolvability(msa, truth, mc, start, ende)
        one = np.where(truth >= 0, 0, -1)                              # a single copy: nothing to compare it with (TA:112)
        assert code_of(lambda: resolvability(msa, one, mc, start=500, ende=1750)) == -1


@pytest.mark.gpu
def test_pipeline_resolved_copies():
    from repeatresolver_amd.max_correlation import max_correlations
    from repeatresolver_amd.pipeline import resolved, resolved_copies
    from repeatresolver_amd.resolution import consensus, open_msa
    rows = ragged()
    sites, windows, con, copies = resolved_copies(rows, parts=3, cov=COV)
    sites0, windows0, con0 = resolved(rows, parts=3, cov=COV)
    assert sites == sites0 and len(windows) == len(windows0) == len(copies) == 3 and np.array_equal(con.matrix, con0.matrix)
    mc = max_correlations(rows, COV)
    with open_msa(rows) as msa:
        for w, w0, c in zip(windows, windows0, copies):
            assert (w.von, w.bis, w.kept_rows, w.cutoff) == (w0.von, w0.bis, w0.kept_rows, w0.cutoff)
            assert np.array_equal(w.kmeans_labels, w0.kmeans_labels) and np.array_equal(w.reldrop_labels, w0.reldrop_labels)
            assert np.array_equal(w.dropoff_labels, w0.dropoff_labels)
            e = consensus(msa, w.kmeans_labels, w.von, w.bis, mc, w.cutoff)
            assert (c.von, c.bis, c.counts) == (e.von, e.bis, None) and c.parts == w.kmeans_parts
            for name in ("part_label", "part_rows", "consensus", "depth", "selected", "diff", "diff_all"):
                assert np.array_equal(getattr(c, name), getattr(e, name)), name
            assert len(c.sequences()) == c.parts and all(set(s) <= set(b"ACGT") for s in c.sequences())
