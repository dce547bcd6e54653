"""No GPU: the semantics of pgr_msa_settle (include/pgr.h, last section: consensus and assignment iterated until no row moves) as
tests/st_checker.py restates them: the hand-made case with two iterations worked out by hand (tests/st_cases.py); the vectorised
checker against the plain one; the conditions of the inputs of tests/test_gpu_settle.py, computed by the checker alone; the
exports, constants and struct sizes; the argument errors, which are refused before the device is touched.  Everything compared is
an integer and compared exactly."""
import ctypes
import inspect

import numpy as np
import pytest

import as_cases as asc
import cs_cases as cs
import st_cases as sc
import st_checker as st


def test_checker_on_the_hand_made_case():
    """6 x 9, labels 0 0 2 2 - 2, every column, thresholds (3, 1), free: the two iterations written out in st_cases, and the third"""
    one = st.settle(cs.HAND_ROWS, sc.hand_labels(), 0, 8, None, 1.0, plain=True, **dict(sc.HAND_ARGS, max_iter=1))
    assert (one["stop"], one["iterations"]) == ("MAX_ITER", 1) and one["labels"].tolist() == sc.HAND_LABELS_AFTER[0]
    assert one["changed"].tolist() == sc.HAND_CHANGED[:1] and one["columns"].tolist() == sc.HAND_COLUMNS
    assert one["compared"].tolist() == asc.HAND_COMPARED and one["mismatches"].tolist() == asc.HAND_MISMATCHES       # iteration 0 is as_cases' case
    assert one["best"].tolist() == asc.HAND_BEST and one["second"].tolist() == asc.HAND_SECOND
    two = sc.expected("hand")
    assert (two["stop"], two["iterations"]) == ("MAX_ITER", 2) and two["labels"].tolist() == sc.HAND_LABELS_AFTER[1]
    assert two["changed"].tolist() == sc.HAND_CHANGED and two["parts_at"].tolist() == [2, 2] and two["ncolumns_at"].tolist() == [8, 8]
    assert two["columns"].tolist() == sc.HAND_COLUMNS and two["part_label"].tolist() == [0, 2]
    assert two["compared"].tolist() == sc.HAND_COMPARED and two["mismatches"].tolist() == sc.HAND_MISMATCHES_1
    assert two["best"].tolist() == sc.HAND_BEST_1 and two["second"].tolist() == sc.HAND_SECOND_1
    assert two["best_mismatches"].tolist() == [min(m) for m in sc.HAND_MISMATCHES_1]
    assert two["second_mismatches"].tolist() == [max(m) for m in sc.HAND_MISMATCHES_1]
    five = st.settle(cs.HAND_ROWS, sc.hand_labels(), 0, 8, None, 1.0, plain=True, **dict(sc.HAND_ARGS, max_iter=5))
    assert (five["stop"], five["iterations"], five["changed"].tolist()) == ("CONVERGED", 3, sc.HAND_CHANGED + [0])
    assert five["labels"].tolist() == sc.HAND_LABELS_AFTER[1]
    # held, the rows of the labelling never move: only row 4 could join, and it ties
    held = st.settle(cs.HAND_ROWS, sc.hand_labels(), 0, 8, None, 1.0, plain=True, **dict(sc.HAND_ARGS, max_iter=5, hold=True))
    assert (held["stop"], held["iterations"], held["labels"].tolist()) == ("CONVERGED", 1, [0, 0, 2, 2, -1, 2])
    # min_depth 3 leaves no column (part 0 has two rows): no iteration, nothing per row
    none = st.settle(cs.HAND_ROWS, sc.hand_labels(), 0, 8, None, 1.0, plain=True, **dict(sc.HAND_ARGS, min_depth=3))
    assert (none["stop"], none["iterations"], none["best"], none["columns"]) == ("NO_COLUMN", 0, None, None)
    assert none["labels"].tolist() == [0, 0, 2, 2, -1, 2]
    # min_compared above the width: the first iteration labels no row, the labelling before it stays
    empty = st.settle(cs.HAND_ROWS, sc.hand_labels(), 0, 8, None, 1.0, plain=True, **dict(sc.HAND_ARGS, min_compared=10))
    assert (empty["stop"], empty["iterations"], empty["changed"].tolist()) == ("EMPTY", 1, [5]) and empty["labels"].tolist() == [0, 0, 2, 2, -1, 2]
    assert empty["best"].tolist() == asc.HAND_BEST


def test_numpy_restatement_equals_the_checker():
    text, mc = cs.random_msa(7, 60, 200)
    rows = [r.tobytes() for r in text]
    labels = (np.arange(60) % 5 - 1).astype(np.int32)                  # four parts and rows in none
    moved = 0
    for von, bis, kw in ((3, 190, dict(min_compared=3, min_margin=1)), (0, 199, dict(min_compared=10, min_margin=2, all_columns=True, hold=True)),
                         (20, 150, dict(min_compared=2, min_margin=0, min_depth=2))):
        a = st.settle(rows, labels, von, bis, mc, 1.0, max_iter=4, plain=True, **kw)
        b = st.settle(text, labels, von, bis, mc, 1.0, max_iter=4, **kw)
        assert (a["stop"], a["iterations"]) == (b["stop"], b["iterations"]) and a["iterations"] > 1
        for name in ("labels", "changed", "parts_at", "ncolumns_at", "part_label", "columns", "mismatches") + st.FIELDS:
            assert np.array_equal(a[name], b[name]), name
        moved += int(a["changed"].sum())
    assert moved > 0


def test_conditions_of_inputs_a_and_b():
    """cs_cases.random_msa(3, 900, 1031), window [0, 1030], the columns over the cutoff 1.0, thresholds (5, 1), min_depth 1,
    max_iter 12.  A: cs_cases.geometry_labels() (parts of 511, 255 and 1 rows); B: 130 parts of one to five rows"""
    hold, free, b = sc.expected("A-hold"), sc.expected("A-free"), sc.expected("B")
    assert (hold["stop"], hold["iterations"]) == ("CONVERGED", 12)
    assert hold["changed"].tolist() == [125, 15, 9, 4, 3, 2, 2, 2, 1, 1, 1, 0]
    assert (free["stop"], free["iterations"]) == ("MAX_ITER", 12) and free["changed"][0] == 413 and (free["changed"] > 0).all()
    for e in (hold, free):
        assert e["ncolumns_at"].tolist() == [260] + [370] * 11 and e["parts_at"].tolist() == [3] * 12
    assert (b["stop"], b["iterations"], b["best"], b["part_label"]) == ("NO_COLUMN", 0, None, None)
    assert np.array_equal(b["labels"], cs.many_parts_labels(900, 130))


def test_conditions_of_input_c():
    """the noisy copies of st_cases: five copies, 900 x 1031, 260 rows seeded"""
    text, truth, seeds, mc = sc.noisy_copies()
    assert text.shape == (900, 1031) and (seeds >= 0).sum() == 260 and sc.share_true(seeds, truth) == (260, 1.0)
    assert set(np.unique(text).tolist()) == set(b"acgtACGT-_ ")
    # C1: a quarter of the seeds wrong.  Free: every row labelled and on its true copy; held: the wrong seeds stay
    assert sc.share_true(sc.c_labels(1), truth) == (260, 0.75)
    for name in ("C1-free", "C1-third-free"):
        e = sc.expected(name)
        assert e["stop"] == "CONVERGED" and sc.share_true(e["labels"], truth) == (900, 1.0)        # (the issue asks for at least 0.99)
    e = sc.expected("C1-hold")
    wrong = sc.c_labels(1) != seeds
    assert wrong.sum() == 65 and np.array_equal(e["labels"][wrong], sc.c_labels(1)[wrong])
    assert sc.share_true(e["labels"], truth) == (900, (900 - 65) / 900)           # 0.928: all but the wrong seeds
    assert sc.expected("C1-third-free")["ncolumns_at"].tolist() == [332, 340] and sc.expected("C1-free")["ncolumns_at"].tolist() == [997, 1020]
    # C2: at least four iterations, and the compared columns shrink between iterations
    e = sc.expected("C2-free")
    assert (e["stop"], e["iterations"]) == ("CONVERGED", 4) and e["changed"].tolist() == [559, 141, 1, 0]
    assert e["ncolumns_at"].tolist() == [936, 864, 864, 864] and e["parts_at"].tolist() == [6, 6, 6, 6]
    # the same with min_depth 2 runs out of columns in its third iteration: what is returned is the second's
    e = sc.expected("C2-depth2")
    assert (e["stop"], e["iterations"]) == ("NO_COLUMN", 2) and e["changed"].tolist() == [560, 141] and e["ncolumns_at"].tolist() == [928, 719]
    assert len(e["columns"]) == 719 and e["best"] is not None
    # C3: the sixth part dies in the first iteration of the free run and stays in the held one
    free, held = sc.expected("C3-free"), sc.expected("C3-hold")
    assert free["parts_at"].tolist() == [6, 5] and free["ncolumns_at"].tolist() == [812, 1020] and free["part_label"].tolist() == [1, 3, 5, 7, 9]
    assert held["parts_at"].tolist() == [6, 6] and held["ncolumns_at"].tolist() == [812, 812] and held["part_label"].tolist() == [1, 3, 5, 7, 9, 11]
    assert (held["labels"] == 11).sum() == 3 and not (free["labels"] == 11).any()
    assert sc.expected("C3-third-free")["parts_at"].tolist() == [6, 5]
    # C4: min_compared above the width: EMPTY after one iteration, the returned labels are the input's
    e = sc.expected("C4-free")
    assert (e["stop"], e["iterations"], e["changed"].tolist()) == ("EMPTY", 1, [260]) and np.array_equal(e["labels"], seeds)
    assert e["best"] is not None and (e["best"] >= 0).sum() > 800


def test_exports_constants_and_structs():
    import os
    import re
    from conftest import ROOT
    from repeatresolver_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgr.h")).read()
    define = {n: v for n, v in re.findall(r"#define (PGR_ST_[A-Z_]+) +([0-9]+)", text)}
    assert define == {"PGR_ST_CONVERGED": "0", "PGR_ST_MAX_ITER": "1", "PGR_ST_EMPTY": "2", "PGR_ST_NO_COLUMN": "3"}
    for name, value in define.items():
        assert getattr(_lib, name) == int(value) and _lib.PGR_ST_NAMES[int(value)] == name[len("PGR_ST_"):]
    lib = _lib.load()
    for name in ("pgr_msa_settle", "pgr_settlement_free", "pgr_last_settle_timing"):
        assert name in _lib.PGR_EXPORTS and getattr(lib, name) is not None and re.search(r"\b%s\(" % name, text)
    assert "pgr_settlement;" in text
    assert ctypes.sizeof(_lib.PgrSettlement) == 4 * 4 + 5 * 8 + 4 + 4 + 6 * 8     # four ints, five pointers, an int and padding, six pointers
    assert ctypes.sizeof(_lib.PgrAssignment) == 3 * 4 + 4 + 6 * 8                  # unchanged
    assert ctypes.sizeof(_lib.PgrConsensus) == 5 * 4 + 4 + 5 * 8 + 8 + 3 * 8       # unchanged


def test_the_thresholds_have_no_default():
    from repeatresolver_amd import pipeline, resolution
    for f in (resolution.settle, pipeline.settled):
        p = inspect.signature(f).parameters
        for name in ("min_compared", "min_margin", "max_iter"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is inspect.Parameter.empty, (f.__name__, name)
    assert inspect.signature(resolution.settle).parameters["hold"].default is False
    assert inspect.signature(pipeline.settled).parameters["hold"].default is True
    with pytest.raises(TypeError):
        resolution.settle(None, [0])


class FakeMsa(ctypes.Structure):
    """struct pgr_msa of csrc/pgr_internal.h with no text behind it: an argument error must not get as far as reading it"""
    _fields_ = [("rows", ctypes.c_int), ("width", ctypes.c_int), ("device", ctypes.c_int), ("text", ctypes.c_void_p)]


def test_argument_errors_need_no_device():
    from repeatresolver_amd import _lib
    lib = _lib.load()
    msa = FakeMsa(6, 20, 0, None)
    h = ctypes.cast(ctypes.pointer(msa), ctypes.c_void_p)
    pi = ctypes.POINTER(ctypes.c_int)

    def call(labels=(0, 0, 2, 2, -1, 2), von=4, bis=11, min_depth=1, min_compared=3, min_margin=1, hold=0, max_iter=5, handle=h, out="fresh"):
        lab = None if labels is None else np.array(labels, np.int32)
        o = _lib.PgrSettlement(rows=77, iterations=77, stop=77, parts=77, ncolumns=77)
        o.labels = ctypes.cast(1, pi)                                  # garbage the call has to zero before anything else
        o.best = ctypes.cast(1, pi)
        rc = lib.pgr_msa_settle(handle, None if lab is None else lab.ctypes.data_as(pi), von, bis, None, 1.0, min_depth, 0, min_compared,
                                min_margin, hold, max_iter, None if out is None else ctypes.byref(o))
        assert out is None or (o.rows, o.iterations, o.stop, o.parts, o.ncolumns, bool(o.labels), bool(o.best)) == (0, 0, 0, 0, 0, False, False)
        return rc

    for what, code in ((dict(out=None), -1), (dict(handle=None), -1), (dict(labels=None), -1),
                       (dict(von=12), -1), (dict(von=-1), -1), (dict(von=-2, bis=-1), -1), (dict(bis=20), -1), (dict(von=20, bis=20), -1),
                       (dict(labels=(0, 0, -2, 2, -1, 2)), -1), (dict(labels=(-1,) * 6), -1),
                       (dict(labels=(0, 0, 2, 2, -1, _lib.PGR_MAX_ROWS)), -5),
                       (dict(max_iter=0), -1), (dict(max_iter=-4), -1), (dict(min_depth=0), -1), (dict(min_compared=-1), -1),
                       (dict(min_margin=-1), -1), (dict(hold=1, max_iter=0), -1)):
        assert call(**what) == code, what                               # (no good call here: the handle has no text)
    assert lib.pgr_last_settle_timing(None) == -1
    lib.pgr_settlement_free(None)
