"""-m gpu: pgr_msa_settle (include/pgr.h; the kernels of pgr_settle_device.hip) through resolution.settle against
tests/st_checker.py, the restatement of the header's loop from the checkers of its two halves, on the inputs whose conditions
tests/test_settle.py pins; and, for the geometry, against the same loop composed from resolution.consensus / assign /
Assignment.labels on the GPU, which tests/test_gpu_consensus.py and tests/test_gpu_assign.py hold to their checkers.  Every field
is an integer or a name and compared exactly; there is no tolerance in this file but the 1e-10 of the connection matrix, which is
host code in doubles (derivation: tests/test_connect.py).

Shapes: a word of the planes is 64 candidate columns; k_st_planes reads groups of 64 rows, four per work-group; k_st_cons has
a work-group per (word, part) whose four waves share the part's rows; k_st_mask a wave per word, 64 parts per step; k_st_dist 64
rows per work-group, tiles of 8 parts, the words dealt to 16 waves; k_st_scan 1024 threads over the label values.  So: 1, 63, 64,
65, 129 and 1027 candidates; 900 rows; 1, 2, 7, 8, 9 and 130 parts; parts of 511, 255, 3, 2 and 1 rows; labels up to 30 000 - 1."""
import functools

import numpy as np
import pytest

import cn_checker as cn
import cs_cases as cs
import st_cases as sc
import st_checker as st
from test_gpu_resolve import COV, ragged

NAMED_ROWS = (63, 64, 65, 127, 128, 255, 256, 899)


def composed(msa, labels, von=None, bis=None, maxcorrs=None, cutoff=1.0, *, min_compared, min_margin, max_iter, min_depth=1,
             all_columns=False, hold=False):
    """the loop of the header from the public calls, on the GPU: a dict as st_checker.settle returns"""
    from repeatresolver_amd.resolution import assign, consensus
    initial = np.asarray(labels, dtype=np.int32)
    lab, history, last, stop = initial.copy(), [], None, "MAX_ITER"
    for _ in range(max_iter):
        con = consensus(msa, lab, von, bis, maxcorrs, cutoff)
        try:
            a = assign(msa, con, min_depth, all_columns)
        except ValueError:
            stop = "NO_COLUMN"
            break
        new = a.labels(min_compared, min_margin, keep=initial if hold else None)
        changed = int((new != lab).sum())
        history.append((changed, con.parts, len(a.columns)))
        last = a
        if changed == 0:
            stop = "CONVERGED"
            break
        if not (new >= 0).any():
            stop = "EMPTY"
            break
        lab = new
    out = {"labels": lab, "stop": stop, "iterations": len(history), "changed": np.array([h[0] for h in history], dtype=np.int32),
           "parts_at": np.array([h[1] for h in history], dtype=np.int32), "ncolumns_at": np.array([h[2] for h in history], dtype=np.int32)}
    for name in ("part_label", "columns") + st.FIELDS:
        out[name] = None if last is None else getattr(last, name)
    return out


def both(msa, labels, *args, **kw):
    """settle against the composition; the rows the kernels' edges fall on, by name"""
    from repeatresolver_amd.resolution import settle
    got, exp = settle(msa, labels, *args, **kw), composed(msa, labels, *args, **kw)
    st.same(got, exp)
    if exp["best"] is not None:
        for r in (r for r in NAMED_ROWS if r < len(exp["labels"])):
            assert [int(getattr(got, n)[r]) for n in st.FIELDS + ("labels",)] == [int(exp[n][r]) for n in st.FIELDS + ("labels",)], r
    return got


@pytest.mark.gpu
def test_the_hand_made_case():
    import ctypes
    from repeatresolver_amd import _lib
    from repeatresolver_amd.resolution import last_settle_timing, open_msa, settle
    with open_msa(cs.HAND_ROWS) as msa:
        one = settle(msa, cs.HAND_LABELS, **dict(sc.HAND_ARGS, max_iter=1))
        assert (one.stop, one.iterations, one.labels.tolist()) == ("MAX_ITER", 1, sc.HAND_LABELS_AFTER[0])
        two = settle(msa, cs.HAND_LABELS, **sc.HAND_ARGS)
        assert (two.stop, two.iterations, two.labels.tolist()) == ("MAX_ITER", 2, sc.HAND_LABELS_AFTER[1])
        assert two.changed.tolist() == sc.HAND_CHANGED and two.parts_at.tolist() == [2, 2] and two.ncolumns_at.tolist() == [8, 8]
        assert two.columns.tolist() == sc.HAND_COLUMNS and two.part_label.tolist() == [0, 2] and two.compared.tolist() == sc.HAND_COMPARED
        assert two.best.tolist() == sc.HAND_BEST_1 and two.second.tolist() == sc.HAND_SECOND_1
        assert two.best_mismatches.tolist() == [min(m) for m in sc.HAND_MISMATCHES_1]
        assert two.second_mismatches.tolist() == [max(m) for m in sc.HAND_MISMATCHES_1]
        st.same(two, sc.expected("hand"))
        t = last_settle_timing()
        assert t["planes_ms"] > 0 and t["iterations_ms"] > 0 and t["all_ms"] >= t["planes_ms"] + t["iterations_ms"] + t["download_ms"]
        for kw in (dict(max_iter=5), dict(max_iter=5, hold=True), dict(min_depth=3), dict(min_compared=10), dict(max_iter=5, min_depth=2),
                   dict(max_iter=5, all_columns=False)):
            kw = dict(sc.HAND_ARGS, **kw)
            got = settle(msa, cs.HAND_LABELS, maxcorrs=cs.hand_maxcorrs(), **kw)
            st.same(got, st.settle(cs.HAND_ROWS, sc.hand_labels(), 0, 8, cs.hand_maxcorrs(), 1.0, plain=True, **kw))
        # the selected columns 0 2 3 7 8: column 2 is out in iteration 0 (part 0 has depth 0 there) and in once row 2 has joined part 0
        assert got.ncolumns_at.tolist() == [4, 5] and got.columns.tolist() == [0, 2, 3, 7, 8] and got.labels.tolist() == [0, 2, 0, 2, -1, 2]
        none = settle(msa, cs.HAND_LABELS, **dict(sc.HAND_ARGS, min_depth=3))
        assert (none.stop, none.iterations, none.best, none.columns, none.part_label) == ("NO_COLUMN", 0, None, None, None)
        assert none.labels.tolist() == [0, 0, 2, 2, -1, 2] and none.changed.shape == (0,)
        raw, lab = _lib.PgrSettlement(), sc.hand_labels()              # the struct itself: without an iteration every array but labels is NULL
        assert _lib.load().pgr_msa_settle(msa.handle, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), -1, -1, None, 1.0, 3, 1, 3, 1, 0, 2,
                                          ctypes.byref(raw)) == 0
        assert (raw.rows, raw.iterations, raw.stop, raw.parts, raw.ncolumns) == (6, 0, _lib.PGR_ST_NO_COLUMN, 0, 0) and bool(raw.labels)
        assert not any(bool(getattr(raw, n)) for n in ("changed", "parts_at", "ncolumns_at", "part_label", "columns") + st.FIELDS)
        _lib.load().pgr_settlement_free(ctypes.byref(raw))
        mc = np.zeros(45)                                              # no column over the cutoff: no candidate at all
        none = settle(msa, cs.HAND_LABELS, maxcorrs=mc, min_compared=1, min_margin=0, max_iter=3)
        assert (none.stop, none.iterations, none.best, none.labels.tolist()) == ("NO_COLUMN", 0, None, [0, 0, 2, 2, -1, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A-hold", "A-free", "B"])
def test_inputs_a_and_b(name):
    from repeatresolver_amd.resolution import open_msa, settle
    text, mc = sc.ab_text()
    labels = cs.many_parts_labels(900, 130) if name == "B" else cs.geometry_labels()
    with open_msa(text) as msa:
        got = settle(msa, labels, 0, 1030, mc, 1.0, hold=name == "A-hold", **sc.AB_ARGS)
    st.same(got, sc.expected(name))
    assert got.stop == {"A-hold": "CONVERGED", "A-free": "MAX_ITER", "B": "NO_COLUMN"}[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(sc.C_CASES))
def test_input_c(name):
    from repeatresolver_amd.resolution import open_msa, settle
    labels, kw = sc.c_args(name)
    with open_msa(sc.noisy_copies()[0]) as msa:
        got = settle(msa, labels, kw.pop("von"), kw.pop("bis"), kw.pop("maxcorrs"), kw.pop("cutoff"), **kw)
    st.same(got, sc.expected(name))


@functools.lru_cache(maxsize=None)
def geometry():
    """900 x 1031 over the full alphabet, a quarter blank; row 65 blank over the window [3, 1029]; rows 70 .. 74 are row 75 again"""
    text = cs.random_msa(1, 900, 1031)[0].copy()
    text[65, 3:1030] = ord(" ")
    text[70:75] = text[75]
    text.setflags(write=False)
    return text


def selecting(columns, width=1031):
    """MaxCorrs that put exactly `columns` over the cutoff 1.0"""
    mc = np.zeros(width * 5)
    mc[5 * np.asarray(columns) + 1] = 2.0
    return mc


def spread_labels(parts, rows=900):
    """`parts` parts of about rows / parts rows each, every eleventh row in none; labels with gaps"""
    lab = (3 * (np.arange(rows) % parts) + 2).astype(np.int32)
    lab[::11] = -1
    return lab


def twin_labels(parts):
    """spread_labels with two of the parts being the twins: {70, 71, 72} under label 1000 and {73, 74, 75} under 1003, six
    identical rows (geometry), so the two consensus are equal and all six rows tie between them; each has depth 3 or 0.  With min_margin 0 they all take the
    lower index and 1003 dies; with min_margin 1 none is sure and both die; held, both stay."""
    if parts < 2:
        return spread_labels(parts)
    lab = spread_labels(parts - 2) if parts > 2 else np.full(900, -1, dtype=np.int32)
    lab[70:73], lab[73:76] = 1000, 1003
    return lab


@pytest.mark.gpu
def test_geometry_candidates():
    """window [3, 1029]: 1, 63, 64, 65, 129 candidates and all 1027; a list with gaps of more than 64 columns; scattered ones"""
    from repeatresolver_amd.resolution import open_msa
    text, window, lab = geometry(), np.arange(3, 1030), spread_labels(4)
    kw = dict(min_compared=1, min_margin=1, max_iter=4)
    with open_msa(text) as msa:
        for n in (1, 63, 64, 65, 129, 1027):
            got = both(msa, lab, 3, 1029, selecting(window[:n]), 1.0, **kw)
            assert got.iterations >= 1 and got.ncolumns_at[0] == n and got.compared[65] == 0
            assert got.labels[65] == (lab[65] if got.stop == "EMPTY" else -1)    # (one column: the four consensus agree, every row ties)
        got = both(msa, lab, 3, 1029, None, 1.0, all_columns=True, hold=True, **kw)
        assert got.ncolumns_at[0] == 1027 and np.array_equal(got.labels[lab >= 0], lab[lab >= 0])
        got = both(msa, lab, 3, 1029, selecting([3, 70, 71, 300, 1000, 1029]), 1.0, **kw)
        assert got.columns is not None and got.compared.max() <= 6
        both(msa, lab, 3, 1029, selecting(window[::5]), 1.0, **dict(kw, min_compared=20, min_margin=2))
        # candidates outside the window do not count
        got = both(msa, lab, 100, 300, selecting([3, 100, 200, 300, 301, 1029]), 1.0, **kw)
        assert got.ncolumns_at[0] == 3


@pytest.mark.gpu
def test_geometry_windows():
    """a window ending in the text's last byte; von of every residue mod 4; a one-column window; the whole width by default"""
    from repeatresolver_amd.resolution import open_msa
    text, lab = geometry(), spread_labels(3)
    kw = dict(min_compared=1, min_margin=1, max_iter=3)
    with open_msa(text) as msa:
        both(msa, lab, 998, 1030, **kw)
        both(msa, lab, **dict(kw, min_compared=100, min_margin=3))
        for von in (4, 5, 6, 7):
            both(msa, lab, von, von + 99, selecting(np.arange(von, von + 100, 3)), 1.0, **kw)
        both(msa, lab, 1030, 1030, **dict(kw, min_margin=0))
        both(msa, lab, 517, 517, **dict(kw, min_margin=0, hold=True))


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 2, 7, 8, 9, 130])
def test_geometry_parts(parts):
    """one part (no second: every row with enough compared joins it), the part tile of 8 and one less and one more, 130 parts
    (17 tiles; three steps of k_st_mask), free and held, min_depth 1, 2 and 3; two of the parts are twins and die in the free runs.  With min_depth 3 the ballot of
    depth >= min_depth keeps some of the 129 candidates and drops others (a quarter of the text is blank: the twins alone drop a
    quarter of them), and what is left goes through the distance and label kernels; with 130 parts of six or seven rows hardly a
    column is left, and none may be"""
    from repeatresolver_amd.resolution import open_msa
    text, lab = geometry(), twin_labels(parts)
    cand = selecting(np.arange(3, 1030, 8))                            # 129 candidates: three words
    runs = []
    with open_msa(text) as msa:
        for kw in (dict(min_margin=0), dict(min_margin=1), dict(min_margin=1, hold=True), dict(min_margin=0, min_depth=2),
                   dict(min_margin=2, min_depth=2, hold=True), dict(min_margin=0, min_depth=3), dict(min_margin=1, min_depth=3, hold=True)):
            got = both(msa, lab, 3, 1029, cand, 1.0, min_compared=5, max_iter=4, **kw)
            if kw.get("min_depth") == 3 and parts == 130:
                assert got.iterations == 0 or got.ncolumns_at[0] < 10
            else:
                assert got.iterations >= 1 and got.parts_at[0] == parts
            assert not kw.get("hold") or (got.parts_at == parts).all()
            if kw.get("min_depth") == 3 and 2 <= parts <= 9:               # a reduced, non-empty set of columns is compared
                assert 0 < got.ncolumns_at[0] < 129 and got.compared.max() > 0
                assert not kw.get("hold") or ((got.ncolumns_at < 129).all() and len(got.columns) == got.ncolumns_at[-1])   # held, the twins stay
            runs.append(got)
    if parts == 1:
        assert all((got.second == -1).all() and (got.second_mismatches == 0).all() for got in runs)
    else:
        for got, left in ((runs[0], parts - 1), (runs[3], parts - 1)) + (((runs[1], parts - 2),) if parts > 2 else ()):
            assert got.iterations > 1 and got.parts_at[1] == left and 1003 not in got.part_label.tolist(), left
        assert runs[0].labels[70:76].tolist() == [1000] * 6 and 1000 in runs[0].part_label.tolist()
    if parts == 2:                                                     # both twins die at once: the labelling before stays
        assert (runs[1].stop, runs[1].iterations) == ("EMPTY", 1) and np.array_equal(runs[1].labels, lab)


@pytest.mark.gpu
def test_long_and_short_parts_and_the_largest_label():
    """cs_cases.geometry_labels(): parts of 511, 255 and 1 rows; then two more of 2 and 3 rows, one under the largest label there
    is; max_iter = 1 is assign and labels exactly; then parts of 511, 255, 3 and 3 rows with min_depth 3, where the two small
    parts have the depth in under half of the columns"""
    from repeatresolver_amd import _lib
    from repeatresolver_amd.resolution import assign, consensus, open_msa, settle
    text, mc = sc.ab_text()
    lab = cs.geometry_labels().copy()
    with open_msa(text) as msa:
        for hold in (False, True):
            got = both(msa, lab, 0, 1030, mc, 1.0, min_compared=5, min_margin=1, max_iter=3, hold=hold)
            assert got.parts_at[0] == 3 and got.part_label.tolist() == [1, 4, 9]
        free = np.nonzero(lab < 0)[0]
        lab[free[:2]] = 20000
        lab[free[2:5]] = _lib.PGR_MAX_ROWS - 1
        for hold in (False, True):
            got = both(msa, lab, 0, 1030, mc, 1.0, min_compared=5, min_margin=1, max_iter=3, hold=hold)
            assert got.parts_at[0] == 5
        assert got.part_label.tolist() == [1, 4, 9, 20000, _lib.PGR_MAX_ROWS - 1]
        for hold in (False, True):
            one = settle(msa, lab, 0, 1030, mc, 1.0, min_compared=5, min_margin=1, max_iter=1, hold=hold)
            a = assign(msa, consensus(msa, lab, 0, 1030, mc, 1.0))
            assert (one.stop, one.iterations) == ("MAX_ITER", 1) and np.array_equal(one.labels, a.labels(5, 1, keep=lab if hold else None))
            assert np.array_equal(one.columns, a.columns) and np.array_equal(one.part_label, a.part_label)
            for name in st.FIELDS:
                assert np.array_equal(getattr(one, name), getattr(a, name)), name
        lab[free[:2]] = -1                                             # no part of two rows; the part of one row gets two more
        lab[free[5:7]] = 9
        selected = int((mc.reshape(-1, 5).max(axis=1) > 1.0).sum())
        for hold in (False, True):
            got = both(msa, lab, 0, 1030, mc, 1.0, min_compared=5, min_margin=1, max_iter=3, min_depth=3, hold=hold)
            assert got.iterations >= 1 and got.parts_at[0] == 4 and 0 < got.ncolumns_at[0] < selected // 2
            assert len(got.columns) > 0 and got.compared.max() > 0
            one = settle(msa, lab, 0, 1030, mc, 1.0, min_compared=5, min_margin=1, max_iter=1, min_depth=3, hold=hold)
            a = assign(msa, consensus(msa, lab, 0, 1030, mc, 1.0), min_depth=3)
            assert np.array_equal(one.columns, a.columns) and np.array_equal(one.labels, a.labels(5, 1, keep=lab if hold else None))
            assert 0 < len(one.columns) == got.ncolumns_at[0] and 0 < one.compared.max() <= len(one.columns)   # the reduced set, compared


@pytest.mark.gpu
def test_an_msa_of_one_row():
    from repeatresolver_amd.resolution import open_msa
    row = b"acgt-_ACGT nN acgtacgt  " * 3
    with open_msa([row]) as msa:
        got = both(msa, [7], 1, len(row) - 2, min_compared=1, min_margin=0, max_iter=3)
        assert (got.stop, got.iterations, got.labels.tolist(), got.best.tolist(), got.second.tolist()) == ("CONVERGED", 1, [7], [0], [-1])
        assert got.best_mismatches.tolist() == [0] and got.compared.tolist() == [len(got.columns)]
        got = both(msa, [7], 1, len(row) - 2, min_compared=len(row), min_margin=0, max_iter=3)
        assert (got.stop, got.labels.tolist()) == ("EMPTY", [7])


def code_of(call):
    from repeatresolver_amd.realigner import PwrError
    try:
        call()
        return 0
    except PwrError as e:
        return e.code


@pytest.mark.gpu
def test_errors_with_a_device_open():
    from repeatresolver_amd import _lib
    from repeatresolver_amd.resolution import open_msa, settle
    text, lab = geometry(), spread_labels(3)
    good = dict(min_compared=1, min_margin=1, max_iter=2)
    top = lab.copy()
    top[0] = _lib.PGR_MAX_ROWS
    low = lab.copy()
    low[5] = -2
    with open_msa(text) as msa:
        for args, kw, code in (((lab, 10, 100), good, 0), ((lab, 100, 10), good, -1), ((lab, 0, 1031), good, -1), ((lab, -1, 5), good, -1),
                               ((np.full(900, -1), 10, 100), good, -1), ((low, 10, 100), good, -1), ((top, 10, 100), good, -5),
                               ((lab, 10, 100), dict(good, max_iter=0), -1), ((lab, 10, 100), dict(good, min_depth=0), -1),
                               ((lab, 10, 100), dict(good, min_compared=-1), -1), ((lab, 10, 100), dict(good, min_margin=-1), -1)):
            assert code_of(lambda: settle(msa, *args, **kw)) == code, (args[1:], kw, code)
        with pytest.raises(ValueError):
            settle(msa, lab[:-1], **good)
        with pytest.raises(ValueError):
            settle(msa, lab, 10, None, **good)
        with pytest.raises(ValueError):
            settle(msa, lab, maxcorrs=np.zeros(7), **good)
        with pytest.raises(TypeError):
            settle(msa, lab, min_compared=1, min_margin=1)


@pytest.mark.gpu
def test_pipeline_settled():
    from repeatresolver_amd.max_correlation import max_correlations
    from repeatresolver_amd.pipeline import assigned, settled
    from repeatresolver_amd.resolution import connect
    rows = ragged()
    text = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)
    mc_, mm = 10, 3
    sites0, windows0, con0, copies0, assignments, recruited, con2 = assigned(rows, parts=3, cov=COV, min_compared=mc_, min_margin=mm)
    # one held iteration is `assigned`
    sites, windows, con, copies, settlements, con1 = settled(rows, parts=3, cov=COV, min_compared=mc_, min_margin=mm, max_iter=1)
    assert sites == sites0 and len(windows) == len(settlements) == 3 and np.array_equal(con.matrix, con0.matrix)
    for w, w0, c, c0, s, a, lab in zip(windows, windows0, copies, copies0, settlements, assignments, recruited):
        assert np.array_equal(w.kmeans_labels, w0.kmeans_labels) and np.array_equal(c.consensus, c0.consensus)
        assert (s.stop, s.iterations) == ("MAX_ITER", 1) and np.array_equal(s.labels, lab) and s.labels.dtype == np.int32
        assert np.array_equal(s.columns, a.columns) and np.array_equal(s.part_label, a.part_label)
        for name in st.FIELDS:
            assert np.array_equal(getattr(s, name), getattr(a, name)), name
    assert np.array_equal(con1.matrix, con2.matrix) and np.array_equal(con1.best, con2.best)
    with pytest.raises(TypeError):
        settled(rows, parts=3, cov=COV, min_compared=mc_, min_margin=mm)     # no default for max_iter
    # settled, held and free, against the checker
    mc = max_correlations(rows, COV)
    for hold in (True, False):
        sites, windows, con, copies, settlements, con3 = settled(rows, parts=3, cov=COV, min_compared=mc_, min_margin=mm, max_iter=8, hold=hold)
        for w, s in zip(windows, settlements):
            st.same(s, st.settle(text, w.kmeans_labels, w.von, w.bis, mc, w.cutoff, mc_, mm, 8, hold=hold))
            inside = w.kmeans_labels >= 0
            assert s.iterations > 1 and (not hold or np.array_equal(s.labels[inside], w.kmeans_labels[inside]))
            assert (s.labels[~inside] >= 0).sum() > 0                  # rows are recruited
        got = connect([s.labels for s in settlements])
        assert np.array_equal(con3.matrix, got.matrix) and np.array_equal(con3.best, got.best) and np.array_equal(con3.mutual, got.mutual)
        exp = cn.connection_matrix([s.labels.tolist() for s in settlements])  # host code in doubles: 1e-10, tests/test_connect.py
        assert con3.matrix.shape == exp.shape and np.abs(con3.matrix - exp).max() <= 1e-10
