"""No GPU: the semantics of pgr_msa_assign (include/pgr.h, last section: every row against the consensus of every part) as
tests/as_checker.py restates them, on the hand-made case of tests/cs_cases.py with every row worked out by hand
(tests/as_cases.py); the vectorised checker against the plain one; Assignment.labels; the exports, constants and struct size;
the argument errors, which are refused before the device is touched; and the conditions of the main input of
tests/test_gpu_assign.py.  Everything compared is an integer and compared exactly."""
import ctypes

import numpy as np
import pytest

import as_cases as asc
import as_checker as ac
import cs_cases as cs
import ta_checker as ta


def test_checker_on_the_hand_made_case():
    """6 x 9, parts {0, 2}: a column that drops out for depth 0, blanks in rows, both gaps, mixed case, three ties, a row in no part"""
    con = ta.consensus(cs.HAND_ROWS, cs.HAND_LABELS, None, None, cs.hand_maxcorrs(), 1.0)
    assert con["consensus"].tolist() == cs.HAND_CONSENSUS and con["depth"].tolist() == cs.HAND_DEPTH
    for selected, columns, compared, mism, best, second in (
            (None, asc.HAND_COLUMNS, asc.HAND_COMPARED, asc.HAND_MISMATCHES, asc.HAND_BEST, asc.HAND_SECOND),
            (cs.HAND_SELECTED, asc.HAND_SEL_COLUMNS, asc.HAND_SEL_COMPARED, asc.HAND_SEL_MISMATCHES, asc.HAND_SEL_BEST, asc.HAND_SEL_SECOND)):
        assert ac.compared_columns(cs.HAND_DEPTH, 0, 8, selected, 1) == columns
        exp = ac.assign(cs.HAND_ROWS, cs.HAND_CONSENSUS, 0, columns)
        assert exp["compared"].tolist() == compared and exp["mismatches"].tolist() == mism
        assert exp["best"].tolist() == best and exp["second"].tolist() == second
        assert exp["best_mismatches"].tolist() == [min(m) for m in mism] and exp["second_mismatches"].tolist() == [max(m) for m in mism]
    assert con["selected"].tolist() == cs.HAND_SELECTED
    assert ac.compared_columns(cs.HAND_DEPTH, 0, 8, None, 2) == [0, 1, 3, 4, 5, 6, 7]        # column 8: part 0 has depth 1
    assert ac.compared_columns(cs.HAND_DEPTH, 0, 8, None, 3) == []
    # nothing compared, and a single part
    one = ac.assign([b"  a", b"c  "], [[0, 0, 1]], 0, [1, 2])
    assert one["compared"].tolist() == [1, 0] and one["best"].tolist() == [0, -1] and one["second"].tolist() == [-1, -1]
    assert one["best_mismatches"].tolist() == [1, 0] and one["second_mismatches"].tolist() == [0, 0] and one["mismatches"].tolist() == [[1], [0]]


def test_numpy_restatement_equals_the_checker():
    text, mc = cs.random_msa(7, 60, 200)
    rows = [r.tobytes() for r in text]
    labels = (np.arange(60) % 5 - 1).astype(np.int32)                  # four parts and rows in none
    ties = nothing = 0
    for von, bis, selected in ((3, 190, True), (0, 199, False), (64, 64, False)):
        con = ta.consensus(rows, labels, von, bis, mc, 1.0)
        assert len(con["part_label"]) == 4
        columns = ac.compared_columns(con["depth"], von, bis, con["selected"] if selected else None, 1)
        assert len(columns) > 0
        exp, got = ac.assign(rows, con["consensus"], von, columns), ac.numpy_assign(text, con["consensus"], von, columns)
        for name in asc.FIELDS + ("mismatches",):
            assert np.array_equal(exp[name], got[name]), name
        some = [59, 0, 17]
        part = ac.numpy_assign(text, con["consensus"], von, columns, rows=some)
        assert np.array_equal(part["mismatches"], exp["mismatches"][some]) and np.array_equal(part["second"], exp["second"][some])
        ties += int(((exp["best"] >= 0) & (exp["best_mismatches"] == exp["second_mismatches"])).sum())
        nothing += int((exp["compared"] == 0).sum())
        single = ac.numpy_assign(text, con["consensus"][:1], von, columns)
        exp1 = ac.assign(rows, con["consensus"][:1], von, columns)
        for name in asc.FIELDS + ("mismatches",):
            assert np.array_equal(exp1[name], single[name]), name
    assert ties > 0 and nothing > 0


def hand_assignment(**over):
    from repeatresolver_amd.resolution import Assignment
    f = {"von": 0, "bis": 9, "part_label": np.array([3, 7, 8], np.int32), "columns": np.arange(10, dtype=np.int32),
         #                      margin 2   margin 1   compared 4   nothing   second -1   a tie
         "compared": np.array([10, 10, 4, 0, 10, 10], np.int32), "best": np.array([1, 2, 0, -1, 2, 0], np.int32),
         "second": np.array([0, 0, 1, -1, -1, 1], np.int32), "best_mismatches": np.array([1, 3, 0, 0, 9, 5], np.int32),
         "second_mismatches": np.array([3, 4, 4, 0, 0, 5], np.int32), "mismatches": None}
    f.update(over)
    return Assignment(**f)


def test_assignment_labels():
    a = hand_assignment()
    exp = {name: getattr(a, name) for name in asc.FIELDS}
    assert a.labels(5, 2).tolist() == [7, -1, -1, -1, 8, -1]           # margin 2 == 2 passes, 1 < 2; compared 4 < 5; second -1: no margin asked
    assert a.labels(4, 2).tolist() == [7, -1, 3, -1, 8, -1]            # compared 4 == 4 passes
    assert a.labels(4, 1).tolist() == [7, 8, 3, -1, 8, -1]
    assert a.labels(11, 0).tolist() == [-1] * 6
    assert a.labels(0, 0).tolist() == [7, 8, 3, -1, 8, 3]              # nothing compared: no label, whatever the thresholds; a tie has margin 0
    keep = np.array([-1, 5, 5, 5, -1, -1], np.int32)
    assert a.labels(5, 2, keep=keep).tolist() == [7, 5, 5, 5, 8, -1]   # keep wins, also over a label and over nothing
    assert a.labels(5, 2).dtype == np.int32 and a.labels(5, 2, keep=keep).dtype == np.int32
    for mc, mm, k in ((5, 2, None), (4, 1, None), (0, 0, keep), (4, 3, keep)):
        assert a.labels(mc, mm, keep=k).tolist() == ac.labels(exp, a.part_label, mc, mm, k).tolist()
    with pytest.raises(TypeError):
        a.labels()                                                     # the thresholds have no default
    with pytest.raises(ValueError):
        a.labels(1, 1, keep=keep[:-1])


def test_exports_constants_and_struct():
    import os
    import re
    from conftest import ROOT
    from repeatresolver_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgr.h")).read()
    define = {n: v for n, v in re.findall(r"#define (PGR_[A-Z_]+) +\(?([0-9 <]+)\)?", text)}
    assert define["PGR_AS_SCRATCH_BYTES"].replace(" ", "") == "64<<20"
    assert _lib.PGR_AS_SCRATCH_BYTES == asc.KERNEL_SCRATCH_BYTES == 64 << 20
    assert int(define["PGR_AS_TILE"]) == _lib.PGR_AS_TILE == asc.KERNEL_TILE
    lib = _lib.load()
    for name in ("pgr_msa_assign", "pgr_assignment_free", "pgr_last_assign_timing"):
        assert name in _lib.PGR_EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.PgrAssignment) == 3 * 4 + 4 + 6 * 8         # three ints and padding, six pointers
    assert ctypes.sizeof(_lib.PgrConsensus) == 5 * 4 + 4 + 5 * 8 + 8 + 3 * 8   # unchanged


class FakeMsa(ctypes.Structure):
    """struct pgr_msa of csrc/pgr_internal.h with no text behind it: an argument error must not get as far as reading it"""
    _fields_ = [("rows", ctypes.c_int), ("width", ctypes.c_int), ("device", ctypes.c_int), ("text", ctypes.c_void_p)]


def test_argument_errors_need_no_device():
    from repeatresolver_amd import _lib
    lib = _lib.load()
    msa = FakeMsa(6, 20, 0, None)
    h = ctypes.cast(ctypes.pointer(msa), ctypes.c_void_p)
    pi = ctypes.POINTER(ctypes.c_int)

    def call(parts=2, von=4, width=8, codes="good", columns=(4, 7, 11), ncolumns=None, handle=h, out="fresh"):
        if isinstance(codes, str):
            codes = np.zeros((max(parts, 1), max(width, 1)), np.uint8) + 4
        cols = None if columns is None else np.array(columns, np.int32)
        o = _lib.PgrAssignment(rows=77, parts=77, ncolumns=77)
        o.compared = ctypes.cast(1, pi)                                # garbage the call has to zero before anything else
        rc = lib.pgr_msa_assign(handle, parts, von, width, None if codes is None else codes.ctypes.data_as(ctypes.c_void_p),
                                (0 if cols is None else len(cols)) if ncolumns is None else ncolumns,
                                None if cols is None else cols.ctypes.data_as(pi), 1, None if out is None else ctypes.byref(o))
        assert out is None or (o.rows, o.parts, o.ncolumns, bool(o.compared), bool(o.mismatches)) == (0, 0, 0, False, False)
        return rc

    bad = np.zeros((2, 8), np.uint8)
    bad[1, 7] = 5
    for what, code in ((dict(out=None), -1), (dict(handle=None), -1), (dict(codes=None), -1), (dict(columns=None, ncolumns=3), -1),
                       (dict(parts=0), -1), (dict(parts=-3), -1), (dict(width=0), -1), (dict(von=-1), -1), (dict(von=13), -1),
                       (dict(von=20, width=1, columns=(20,)), -1), (dict(codes=bad), -1),
                       (dict(columns=()), -1), (dict(ncolumns=-1), -1), (dict(columns=(4, 7, 7)), -1), (dict(columns=(7, 4)), -1),
                       (dict(columns=(3, 4)), -1), (dict(columns=(4, 12)), -1), (dict(parts=_lib.PGR_MAX_ROWS + 1, width=2, columns=(4, 5)), -5)):
        assert call(**what) == code, what                               # (no good call here: the handle has no text)
    assert lib.pgr_last_assign_timing(None) == -1
    lib.pgr_assignment_free(None)


def test_conditions_of_the_main_gpu_input():
    """ragged(31) of tests/test_gpu_resolve.py and one row of gaps, the checker chain's k-means labels, cutoff 10.0: what
    tests/test_gpu_assign.py relies on, computed by the checkers alone"""
    rows, text, mc, wins = asc.main_input()
    assert text.shape == (241, 900) and rows[240] == b"-" * 900
    seen = []
    for w in wins:
        exp, lab = w["exp"], w["labels"]
        assert len(w["con"]["part_label"]) == 4 and (w["con"]["consensus"][:, np.array(w["columns"]) - w["von"]] < 4).all()
        index = {int(x): i for i, x in enumerate(w["con"]["part_label"])}
        inside = np.nonzero(lab >= 0)[0]
        own = sum(1 for r in inside if exp["best"][r] == index[int(lab[r])])
        tie = (exp["best"] >= 0) & (exp["best_mismatches"] == exp["second_mismatches"])
        assert tie.sum() >= 1 and tie[240] and (exp["compared"] == 0).sum() >= 1
        assert exp["compared"][240] == len(w["columns"]) == exp["best_mismatches"][240] and exp["best"][240] == 0 and exp["second"][240] == 1
        seen.append((len(w["columns"]), len(inside), own, int(((lab < 0) & (exp["compared"] > 0)).sum()), int(tie.sum()),
                     int((exp["compared"] == 0).sum())))
    # compared columns (= the selected ones: every part has depth there), labelled rows, of them nearest to their own part,
    # unlabelled rows with something compared, ties, rows with nothing compared
    assert seen == [(50, 108, 108, 85, 4, 48), (41, 144, 144, 90, 1, 7), (37, 96, 96, 62, 2, 83)]
    assert [len(w["con"]["selected"]) for w in wins] == [50, 41, 37]
