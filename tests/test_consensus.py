"""No GPU: the semantics of the per-copy consensus (include/pgr.h, bottom section) as tests/ta_checker.py restates them from
TransposonAssessment.py ("TA:"), on hand-made inputs whose outcome is plain; the host parts of the library against the checker
(pgr_resolvability, resolution.transposon_resolution_quality, resolution.write_copies); and the conditions of the main input of
tests/test_gpu_consensus.py.  Everything compared is an integer and compared exactly."""
import ctypes

import numpy as np
import pytest

import cs_cases as cs
import ta_checker as ta


def test_checker_on_the_hand_made_case():
    """6 x 9: an a/c tie, a base/'-' tie, a column of depth 0, mixed case and '_', labels {0, 2} with a gap and a row in no part"""
    exp = ta.consensus(cs.HAND_ROWS, cs.HAND_LABELS, None, None, cs.hand_maxcorrs(), 1.0)
    assert (exp["von"], exp["bis"]) == (0, 8)
    assert exp["part_label"].tolist() == [0, 2] and exp["part_rows"].tolist() == [2, 3]
    assert exp["consensus"].tolist() == cs.HAND_CONSENSUS and exp["depth"].tolist() == cs.HAND_DEPTH
    assert exp["counts"][0, 0].tolist() == [1, 1, 0, 0, 0] and exp["counts"][0, 1].tolist() == [0, 0, 1, 0, 1]      # the two ties
    assert exp["counts"][0, 2].tolist() == [0, 0, 0, 0, 0] and exp["counts"][1, 4].tolist() == [1, 0, 0, 0, 2]
    assert exp["counts"][:, :, 3].sum() == 2 + 1 + 2 + 2 + 2                                                    # no t of the unlabelled row
    assert exp["selected"].tolist() == cs.HAND_SELECTED
    assert exp["diff"].tolist() == [[0, cs.HAND_DIFF], [cs.HAND_DIFF, 0]]
    assert exp["diff_all"].tolist() == [[0, cs.HAND_DIFF_ALL], [cs.HAND_DIFF_ALL, 0]]
    assert ta.tied_columns(exp["counts"]) == 3
    sub = ta.consensus(cs.HAND_ROWS, cs.HAND_LABELS, 2, 6)                                                      # a window, no MaxCorrs
    assert sub["consensus"].tolist() == [r[2:7] for r in cs.HAND_CONSENSUS] and sub["selected"].tolist() == [2, 3, 4, 5, 6]
    assert sub["diff"].tolist() == sub["diff_all"].tolist() == [[0, 3], [3, 0]]
    assert ta.load_labels(["0\n", "\n", "12\n"]) == [0, None, 12] and ta.window_of(503, 1754) == (100, 349)


def test_numpy_restatement_equals_the_checker():
    """cs_cases.numpy_consensus, which stands in for the checker on the one input too large for its loops"""
    text, _ = cs.random_msa(2, 60, 70)
    labels = cs.many_parts_labels(60, 17)
    exp = ta.consensus([r.tobytes() for r in text], labels, 3, 66)
    kon, depth, d_all = cs.numpy_consensus(text, labels, 3, 66)
    assert np.array_equal(kon, exp["consensus"]) and np.array_equal(depth, exp["depth"]) and np.array_equal(d_all, exp["diff_all"])
    assert (exp["depth"] == 0).any() and ta.tied_columns(exp["counts"]) > 0


def c_resolvability(diff):
    from repeatresolver_amd import _lib
    lib = _lib.load()
    d = np.ascontiguousarray(diff, dtype=np.int32)
    P = len(d)
    pi = ctypes.POINTER(ctypes.c_int)
    u, m, l = np.zeros(11, dtype=np.int32), np.zeros(max(P, 1), dtype=np.int32), np.zeros(max(P, 1), dtype=np.int32)
    rc = lib.pgr_resolvability(P, d.ctypes.data_as(pi), u.ctypes.data_as(pi), m.ctypes.data_as(pi), l.ctypes.data_as(pi))
    return rc, u.tolist(), m.tolist(), l.tolist()


def test_resolvability_against_the_checker():
    from repeatresolver_amd.realigner import PwrError
    from repeatresolver_amd.resolution import unique_parts
    rng = np.random.default_rng(11)
    quirk = False
    for P, top in ((2, 4), (3, 12), (7, 14), (40, 30), (5, 1)):
        for _ in range(4):
            d = rng.integers(0, top + 1, size=(P, P))
            d = np.triu(d, 1) + np.triu(d, 1).T
            summe, smallest, returned = ta.resolvability(d.tolist())
            assert c_resolvability(d) == (0, summe, smallest, returned)
            u, m, l = unique_parts(d)
            assert (u, m.tolist(), l.tolist()) == (summe, smallest, returned)
            assert summe == [sum(1 for s in smallest if s > t) for t in range(11)]
            quirk |= smallest != returned
    assert quirk                                                      # what the script returns is not the smallest diff (TA:112)
    plain = [[0, 3, 7], [3, 0, 12], [7, 12, 0]]
    assert c_resolvability(plain) == (0, [3, 3, 3, 1, 1, 1, 1, 0, 0, 0, 0], [3, 3, 7], [7, 12, 12])
    for few in ([[0]], np.zeros((0, 0))):
        assert c_resolvability(few)[0] == -1
        with pytest.raises(PwrError) as e:
            unique_parts(few)
        assert e.value.code == -1
    with pytest.raises(NameError):
        ta.resolvability([[0]])


def test_transposon_resolution_quality():
    from repeatresolver_amd.resolution import resolution_quality, transposon_resolution_quality
    truth = np.arange(90) // 30
    assert transposon_resolution_quality(truth, truth) == ta.resolution_quality(truth, truth) == (3, 0, [3] * 10)
    rng = np.random.default_rng(4)
    for k in (2, 3, 6):
        for _ in range(5):
            t = rng.integers(-1, 5, size=120)
            lab = np.where(rng.random(120) < 0.2, -1, (t % k + (rng.random(120) < 0.3)) % k)
            assert transposon_resolution_quality(t, lab) == ta.resolution_quality(t, lab)
    # Rows of a truth group left at -1.  TA's group keeps them (TA:165, TA:178), the SDA function first restricts the truth to the
    # labelled rows.  Where some rows of the group remain, the normalisation of TA:191-195 divides the group's size out again and
    # both give the same; where the whole group is left out, TA keeps a zero row for it -- and its scan (TA:230-242) finds
    # maxi = 0.0 = max(Matrix3[0]) for the zero row 0: a true positive at no confidence level -- while SDA has no such copy.
    truth = np.array([0] * 40 + [1] * 40)
    labels = np.array([0] * 10 + [-1] * 30 + [0] * 20 + [1] * 20)
    assert transposon_resolution_quality(truth, labels) == ta.resolution_quality(truth, labels) == resolution_quality(truth, labels)
    truth = np.array([0] * 10 + [1] * 20 + [2] * 20)
    labels = np.array([-1] * 10 + [0] * 20 + [1] * 20)
    got, sda = transposon_resolution_quality(truth, labels), resolution_quality(truth, labels)
    assert got == ta.resolution_quality(truth, labels) == (3, 0, [2] * 10) and sda == (2, 0, [2] * 10)
    assert transposon_resolution_quality([0, 0, None, 1, 1], [0, None, 0, 1, 1]) == ta.resolution_quality([0, 0, None, 1, 1], [0, None, 0, 1, 1])
    with pytest.raises(ValueError):
        transposon_resolution_quality([0, 1], [-1, -1])


def hand_consensus():
    from repeatresolver_amd.resolution import Consensus
    e = ta.consensus(cs.HAND_ROWS, cs.HAND_LABELS, None, None, cs.hand_maxcorrs(), 1.0)
    return Consensus(von=e["von"], bis=e["bis"], part_label=e["part_label"], part_rows=e["part_rows"], consensus=e["consensus"],
                     depth=e["depth"], counts=e["counts"], selected=e["selected"], diff=e["diff"], diff_all=e["diff_all"])


def test_sequences_and_write_copies_round_trip(tmp_path):
    from repeatresolver_amd.resolution import write_copies
    con = hand_consensus()
    assert con.parts == 2 and con.sequences() == cs.HAND_SEQUENCES
    path = tmp_path / "copies.fasta"
    write_copies(str(path), con, "MSA")
    lines = path.read_bytes().split(b"\n")
    assert lines == [b">MSA_0_8_copy0 rows=2", cs.HAND_SEQUENCES[0], b">MSA_0_8_copy2 rows=3", cs.HAND_SEQUENCES[1], b""]
    back = {int(h.split(b"copy")[1].split()[0]): s for h, s in zip(lines[0:-1:2], lines[1::2])}                  # read back: label -> sequence
    assert back == dict(zip(con.part_label.tolist(), con.sequences()))


def test_exports_and_constants():
    """the constants tests cite are the header's, and the names of this section are exported"""
    import os
    import re
    from conftest import ROOT
    from repeatresolver_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgr.h")).read()
    define = {n: v for n, v in re.findall(r"#define (PGR_[A-Z_]+) +\(?([0-9 <]+)\)?", text)}
    assert int(define["PGR_CS_TILE"]) == cs.KERNEL_TILE == _lib.PGR_CS_TILE
    assert int(define["PGR_CS_ROWS"]) == cs.KERNEL_ROWS == _lib.PGR_CS_ROWS
    assert define["PGR_CS_SCRATCH_INTS"].replace(" ", "") == "1<<25" and cs.KERNEL_SCRATCH_INTS == _lib.PGR_CS_SCRATCH_INTS == 1 << 25
    assert int(define["PGR_MAX_ROWS"]) == _lib.PGR_MAX_ROWS
    lib = _lib.load()
    for name in ("pgr_msa_consensus", "pgr_consensus_free", "pgr_last_consensus_timing", "pgr_resolvability"):
        assert name in _lib.PGR_EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.PgrConsensus) == 5 * 4 + 4 + 5 * 8 + 8 + 3 * 8      # five ints and padding, five pointers, int and padding, three pointers


def test_conditions_of_the_main_gpu_input():
    """ragged(31) of tests/test_gpu_resolve.py with the oracle's MaxCorrs and cutoff 10.0, windows [von, bis] inclusive: what
    tests/test_gpu_consensus.py relies on, computed by the checker alone"""
    from test_gpu_resolve import SITES, checker_chain
    rows, mc, chain = checker_chain()
    colmax = mc.reshape(-1, 5).max(axis=1)
    assert len(colmax) == 900 and int((colmax > cs.CUTOFF).sum()) == 160
    assert np.abs(colmax - cs.CUTOFF).min() > 0.3                      # no column is near the cutoff
    nsel, smallest = [], []
    for (von, bis), c in zip(zip(SITES[:-1], SITES[1:]), chain):
        exp = ta.consensus(rows, c["km"]["labels"], von, bis, mc, cs.CUTOFF)
        assert len(exp["part_label"]) == 4 and ta.tied_columns(exp["counts"]) == 0
        nsel.append(len(exp["selected"]))
        smallest.append(int(exp["diff_all"][~np.eye(4, dtype=bool)].min()))
        assert ta.selected_columns(mc, von, bis, cs.CUTOFF) == [x for x in range(von, bis + 1) if colmax[x] > cs.CUTOFF]
    assert nsel == [50, 41, 37] and smallest == [20, 15, 11]
