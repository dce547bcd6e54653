"""-m gpu: pgr_msa_assign (include/pgr.h; k_as_planes, k_as_dist, k_as_best of pgr_assign_device.hip) through
resolution.assign_sequences / assign against tests/as_checker.py, the plain restatement of the header's semantics (the reference
has no counterpart), and for the larger inputs against its vectorised form, which tests/test_assign.py compares with the plain
one.  compared, best, second, both counts and the matrix are integers and compared exactly; there is no tolerance in this file
but the 1e-10 of the connection matrix, which is host code in doubles (derivation: tests/test_connect.py).

Shapes: a word of the planes is 64 compared columns; k_as_planes reads groups of 64 rows, four groups per work-group;
k_as_dist has 64 rows per work-group, tiles of as_cases.KERNEL_TILE = 8 parts (padded with zero planes to whole tiles) and deals
the words to 16 waves; a range of rows holds KERNEL_SCRATCH_BYTES.  So: 1, 63, 64, 65 and 129 compared columns (fewer words than
waves) and 1027 (17 words: one wave gets two); 900 rows (14 work-groups and 4 rows; 3 groups of 256 and 132); 1, 2, 7, 8, 9 and
130 parts (16 tiles and 2 parts); 4096 columns (64 words: four per wave) x 16 000 rows x 640 parts, which is two ranges of rows."""
import functools

import numpy as np
import pytest

import as_cases as asc
import as_checker as ac
import cn_checker as cn
import cs_cases as cs
from test_gpu_resolve import COV, ragged


@pytest.mark.gpu
def test_the_hand_made_case():
    from repeatresolver_amd.resolution import assign, consensus, open_msa
    with open_msa(cs.HAND_ROWS) as msa:
        con = consensus(msa, cs.HAND_LABELS, maxcorrs=cs.hand_maxcorrs())
        assert con.consensus.tolist() == cs.HAND_CONSENSUS and con.depth.tolist() == cs.HAND_DEPTH
        for kw, columns, compared, mism, best, second in (
                (dict(all_columns=True), asc.HAND_COLUMNS, asc.HAND_COMPARED, asc.HAND_MISMATCHES, asc.HAND_BEST, asc.HAND_SECOND),
                (dict(), asc.HAND_SEL_COLUMNS, asc.HAND_SEL_COMPARED, asc.HAND_SEL_MISMATCHES, asc.HAND_SEL_BEST, asc.HAND_SEL_SECOND)):
            a = assign(msa, con, matrix=True, **kw)
            assert (a.von, a.bis) == (0, 8) and a.part_label.tolist() == [0, 2] and a.columns.tolist() == columns
            assert a.compared.tolist() == compared and a.mismatches.tolist() == mism
            assert a.best.tolist() == best and a.second.tolist() == second
            assert a.best_mismatches.tolist() == [min(m) for m in mism] and a.second_mismatches.tolist() == [max(m) for m in mism]
            asc.same(a, ac.assign(cs.HAND_ROWS, cs.HAND_CONSENSUS, 0, columns))
        assert assign(msa, con, min_depth=2, all_columns=True).columns.tolist() == [0, 1, 3, 4, 5, 6, 7]
        with pytest.raises(ValueError):
            assign(msa, con, min_depth=3, all_columns=True)
        assert a.labels(3, 1, keep=np.array([0, 0, 2, 2, -1, 2])).tolist() == [0, 0, 2, 2, -1, 2]      # row 4 ties: it stays out


@pytest.mark.gpu
def test_the_windows_and_the_whole_width_of_the_main_input():
    from repeatresolver_amd.resolution import assign, consensus, last_assign_timing, open_msa
    rows, text, mc, wins = asc.main_input()
    with open_msa(text) as msa:
        for w in wins:
            con = consensus(msa, w["labels"], w["von"], w["bis"], mc, cs.CUTOFF)
            assert np.array_equal(con.consensus, w["con"]["consensus"]) and np.array_equal(con.depth, w["con"]["depth"])
            a = assign(msa, con, matrix=True)
            assert a.columns.tolist() == w["columns"] and np.array_equal(a.part_label, w["con"]["part_label"])
            asc.same(a, w["exp"])
        t = last_assign_timing()
        assert t["planes_ms"] > 0 and t["dist_best_ms"] > 0 and t["all_ms"] >= t["planes_ms"] + t["dist_best_ms"] + t["download_ms"]
        labels = np.arange(len(rows), dtype=np.int32) % 7              # the whole width, every column: rows blank at their ends
        con = consensus(msa, labels)
        a = assign(msa, con, all_columns=True, matrix=True)
        columns = ac.compared_columns(con.depth, 0, 899, None, 1)
        assert a.columns.tolist() == columns and len(columns) > 800
        exp = ac.assign(rows, con.consensus, 0, columns)
        asc.same(a, exp)
        assert len(set(exp["compared"].tolist())) > 50 and (exp["compared"] == 0).any() and len(set(exp["best"].tolist())) > 2   # (of the input)


@functools.lru_cache(maxsize=None)
def geometry():
    """900 x 1031 over the full alphabet, a quarter blank; row 65 blank over the window [3, 1029]; the codes of 130 random parts,
    of which parts 0 and 1 are both row 64's own symbols over the whole width (its blanks as code 0): identical codes"""
    text = cs.random_msa(1, 900, 1031)[0].copy()
    text[65, 3:1030] = ord(" ")
    codes = asc.random_codes(12, 130, 1031)
    lut = np.full(256, 0, dtype=np.uint8)
    for ch, k in ac.SYMBOL.items():
        lut[ord(ch)] = k
    codes[0] = codes[1] = lut[text[64]]
    text.setflags(write=False)
    codes.setflags(write=False)
    return text, codes


def geometry_case(msa, text, codes, von, width, columns, parts):
    """one call against the numpy checker, the matrix included; the rows the kernels' edges fall on, by name"""
    from repeatresolver_amd.resolution import assign_sequences
    c = codes[:parts, von:von + width]
    a = assign_sequences(msa, von, c, columns, matrix=True)
    exp = ac.numpy_assign(text, c, von, columns)
    asc.same(a, exp)
    assert (a.von, a.bis) == (von, von + width - 1) and a.part_label.tolist() == list(range(parts))
    for r in (63, 64, 65, 127, 128, 255, 256, 895, 896, 899):
        assert a.mismatches[r].tolist() == exp["mismatches"][r].tolist() and a.best[r] == exp["best"][r] and a.second[r] == exp["second"][r], r
    return a, exp


@pytest.mark.gpu
def test_geometry_columns():
    """window [3, 1029]: 1, 63, 64, 65, 129 compared columns and all 1027; a list with gaps of more than 64 columns"""
    from repeatresolver_amd.resolution import open_msa
    text, codes = geometry()
    window = np.arange(3, 1030)
    with open_msa(text) as msa:
        for n in (1, 63, 64, 65, 129, 1027):
            a, exp = geometry_case(msa, text, codes, 3, 1027, window[:n], 4)
            assert (a.compared[65], a.best[65], a.second[65], a.best_mismatches[65], a.second_mismatches[65]) == (0, -1, -1, 0, 0)
            assert a.mismatches[65].tolist() == [0, 0, 0, 0]
            assert (a.best[64], a.second[64], a.best_mismatches[64], a.second_mismatches[64]) == ((0, 1, 0, 0) if a.compared[64] else (-1, -1, 0, 0))
            assert a.compared.max() <= n and (n < 64 or a.compared.max() > n // 2)
        assert a.compared[64] > 600
        a, exp = geometry_case(msa, text, codes, 3, 1027, [3, 70, 71, 300, 1000, 1029], 4)
        assert a.compared.max() == 6
        a, exp = geometry_case(msa, text, codes, 3, 1027, window[::5], 4)      # 206 scattered columns
        assert (exp["compared"] == 0).sum() >= 1


@pytest.mark.gpu
def test_geometry_windows():
    """a window ending in the text's last column (the last byte of the last row is read); von with every residue mod 4; a
    one-column window"""
    from repeatresolver_amd.resolution import open_msa
    text, codes = geometry()
    with open_msa(text) as msa:
        geometry_case(msa, text, codes, 998, 33, np.arange(998, 1031), 3)
        geometry_case(msa, text, codes, 0, 1031, np.arange(0, 1031), 3)
        for von in (4, 5, 6, 7):
            geometry_case(msa, text, codes, von, 100, np.arange(von, von + 100, 3), 5)
        geometry_case(msa, text, codes, 1030, 1, [1030], 2)
        geometry_case(msa, text, codes, 517, 1, [517], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 2, asc.KERNEL_TILE - 1, asc.KERNEL_TILE, asc.KERNEL_TILE + 1, 130])
def test_geometry_parts(parts):
    """one part (no second), two parts with identical codes, the part tile and one less and one more, 130 parts (17 tiles, the last of two parts)"""
    from repeatresolver_amd.resolution import open_msa
    text, codes = geometry()
    with open_msa(text) as msa:
        a, exp = geometry_case(msa, text, codes, 3, 1027, np.arange(3, 1030, 8), parts)      # 129 columns: three words
    if parts == 1:
        assert (a.second == -1).all() and (a.second_mismatches == 0).all() and set(a.best.tolist()) == {0, -1}
    else:
        assert a.compared[64] > 50 and (a.best[64], a.second[64], a.best_mismatches[64], a.second_mismatches[64]) == (0, 1, 0, 0)
        assert np.array_equal(a.mismatches[:, 0], a.mismatches[:, 1])                       # identical codes: equal counts in every row
        assert not (a.best == 1).any()                                                      # and never the higher index first
        assert np.array_equal(a.second[a.best == 0], np.ones((a.best == 0).sum(), np.int32))
    if parts == 2:
        some = a.compared > 0
        assert (a.best[some] == 0).all() and (a.second[some] == 1).all() and np.array_equal(a.best_mismatches, a.second_mismatches)
    if parts > asc.KERNEL_TILE:
        assert (a.best >= asc.KERNEL_TILE).any() and (a.second >= asc.KERNEL_TILE).any()


@pytest.mark.gpu
def test_an_msa_of_one_row():
    from repeatresolver_amd.resolution import assign_sequences, open_msa
    row = b"acgt-_ACGT nN acgtacgt  " * 3
    codes = asc.random_codes(2, 3, len(row) - 2)
    with open_msa([row]) as msa:
        a = assign_sequences(msa, 1, codes, np.arange(1, len(row) - 1), part_label=[4, 9, 2], matrix=True)
    asc.same(a, ac.assign([row], codes, 1, list(range(1, len(row) - 1))))
    assert a.compared.tolist() == [sum(1 for ch in row[1:-1] if ac.symbol(ch) <= 4)] and a.part_label.tolist() == [4, 9, 2]
    assert a.labels(1, 0).tolist() == [[4, 9, 2][a.best[0]]]


@pytest.mark.gpu
def test_two_ranges_of_rows():
    """16 000 rows x 4 200 columns, 640 parts of random codes, 4 096 compared columns = 64 words: a row takes 32 * 64 + 4 * 640 =
    4 608 bytes of scratch, so KERNEL_SCRATCH_BYTES = 64 MiB holds 14 563 rows: two ranges, 14 563 and 1 437 rows.  compared for
    all rows; everything else for the 300 rows on either side of the boundary, the first and last 100 and 500 random rows,
    against as_checker.numpy_assign (the whole product is too slow for one core, and range errors live at the boundaries)."""
    from repeatresolver_amd.resolution import assign_sequences, open_msa
    T, W, parts, von, width, n = 16000, 4200, 640, 50, 4130, 4096
    per_range = asc.KERNEL_SCRATCH_BYTES // (32 * ((n + 63) // 64) + 4 * parts)
    assert per_range == 14563 and per_range < T <= 2 * per_range
    text = asc.quick_text(8, T, W)
    codes = asc.random_codes(9, parts, width)
    rng = np.random.default_rng(10)
    columns = von + np.sort(rng.choice(width, size=n, replace=False))
    assert columns[0] >= von and columns[-1] <= von + width - 1 and len(set(columns.tolist())) == n
    with open_msa(text) as msa:
        a = assign_sequences(msa, von, codes, columns, matrix=True)
    lut = np.full(256, 5, dtype=np.uint8)
    for ch, k in ac.SYMBOL.items():
        lut[ord(ch)] = k
    assert np.array_equal(a.compared, (lut[text[:, columns]] <= 4).sum(axis=1))
    edges = [b for b in range(per_range, T, per_range)]
    assert edges == [per_range]
    rows = set(range(100)) | set(range(T - 100, T)) | set(rng.choice(T, size=500, replace=False).tolist())
    for b in edges:
        rows |= set(range(b - 300, b + 300))
    rows = np.array(sorted(rows))
    asc.same(a, ac.numpy_assign(text, codes, von, columns, rows=rows), rows=rows)
    assert a.mismatches.shape == (T, parts) and (a.best[rows] >= 0).all() and len(set(a.best.tolist())) > 300


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
    from repeatresolver_amd.resolution import assign_sequences, open_msa
    text, codes = geometry()
    good = codes[:3, 10:110]
    bad = good.copy()
    bad[2, 99] = 5
    with open_msa(text) as msa:
        for von, c, columns, code in ((10, good, [10, 50, 109], 0), (10, bad, [10, 50, 109], -1), (10, good, [], -1), (10, good, [10, 10], -1),
                                      (10, good, [50, 10], -1), (10, good, [9, 10], -1), (10, good, [10, 110], -1), (-1, good, [0, 5], -1),
                                      (932, good, [940], -1), (931, good, [931, 1030], 0), (10, good[:0], [10], -1),
                                      (10, np.zeros((3, 0), np.uint8), [10], -1),
                                      (10, np.zeros((_lib.PGR_MAX_ROWS + 1, 2), np.uint8), [10, 11], -5)):
            assert code_of(lambda: assign_sequences(msa, von, c, columns)) == code, (von, columns, code)
        with pytest.raises(ValueError):
            assign_sequences(msa, 10, good[0], [10])
        with pytest.raises(ValueError):
            assign_sequences(msa, 10, good, [[10, 11]])
        with pytest.raises(ValueError):
            assign_sequences(msa, 10, good, [10], part_label=[1, 2])
        columns = np.arange(10, 110, 2)
        with_matrix, without = assign_sequences(msa, 10, good, columns, matrix=True), assign_sequences(msa, 10, good, columns)
        assert without.mismatches is None and with_matrix.mismatches.shape == (900, 3)
        for name in asc.FIELDS:
            assert np.array_equal(getattr(with_matrix, name), getattr(without, name)), name
        asc.same(without, ac.numpy_assign(text, good, 10, columns), matrix=False)


@pytest.mark.gpu
def test_pipeline_assigned():
    from repeatresolver_amd.max_correlation import max_correlations
    from repeatresolver_amd.pipeline import assigned, resolved_copies
    from repeatresolver_amd.resolution import assign, connect, open_msa
    rows = ragged()
    mc_, mm = 10, 3
    sites, windows, con, copies, assignments, recruited, con2 = assigned(rows, parts=3, cov=COV, min_compared=mc_, min_margin=mm)
    sites0, windows0, con0, copies0 = resolved_copies(rows, parts=3, cov=COV)
    assert sites == sites0 and len(windows) == len(assignments) == len(recruited) == 3 and np.array_equal(con.matrix, con0.matrix)
    with pytest.raises(TypeError):
        assigned(rows, parts=3, cov=COV)                               # no default thresholds
    with open_msa(rows) as msa:
        for w, w0, c, c0, a, lab in zip(windows, windows0, copies, copies0, assignments, recruited):
            assert np.array_equal(w.kmeans_labels, w0.kmeans_labels) and (w.von, w.bis, w.kept_rows) == (w0.von, w0.bis, w0.kept_rows)
            for name in ("part_label", "consensus", "depth", "selected", "diff"):
                assert np.array_equal(getattr(c, name), getattr(c0, name)), name
            e = assign(msa, c)
            assert a.mismatches is None and np.array_equal(a.columns, e.columns) and np.array_equal(a.part_label, c.part_label)
            for name in asc.FIELDS:
                assert np.array_equal(getattr(a, name), getattr(e, name)), name
            text = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)
            asc.same(a, ac.numpy_assign(text, c.consensus, c.von, a.columns), matrix=False)
            assert np.array_equal(lab, a.labels(mc_, mm, keep=w.kmeans_labels)) and lab.dtype == np.int32
            inside = w.kmeans_labels >= 0
            assert np.array_equal(lab[inside], w.kmeans_labels[inside]) and (lab[~inside] >= 0).sum() > 0      # rows are recruited
    got = connect(recruited)
    assert np.array_equal(con2.matrix, got.matrix) and np.array_equal(con2.best, got.best) and np.array_equal(con2.mutual, got.mutual)
    exp = cn.connection_matrix([l.tolist() for l in recruited])        # the connection is host code in doubles: 1e-10, tests/test_connect.py
    assert con2.matrix.shape == exp.shape and np.abs(con2.matrix - exp).max() <= 1e-10 and cn.decided(exp)
    best, conf, mutual = cn.best_columns(exp)
    assert np.array_equal(con2.best, best) and np.array_equal(con2.mutual, mutual) and np.abs(con2.confidence - conf).max() <= 1e-10
