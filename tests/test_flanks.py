"""Flank labellings (include/pfl.h), everything that needs no GPU: the checker against a brute-force edit distance, the host
functions (pfl_neighbours, pfl_cluster, the files, the refusals) against the checker and hand-made cases, and the checker's
distances recovering the copies of toy_a and toy_b."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import fl_checker as fc


def lib():
    from repeatresolver_amd import _lib
    return _lib.load()


# ---- the checker itself ----
def brute(P, T):
    """min over y of the edit distance of P and T[:y], by the textbook recursion"""
    @functools.lru_cache(maxsize=None)
    def lev(x, y):
        if x == 0 or y == 0:
            return x + y
        return min(lev(x - 1, y) + 1, lev(x, y - 1) + 1, lev(x - 1, y - 1) + (P[x - 1] != T[y - 1]))
    return min(lev(len(P), y) for y in range(len(T) + 1))


def test_checker_equals_brute_force_on_short_sequences():
    seqs = [bytes(s) for n in range(0, 6) for s in itertools.product(b"ac", repeat=n)]
    rng = np.random.default_rng(5)
    pairs = [(p, t) for p in seqs for t in seqs]
    pairs += [tuple(bytes(rng.choice(list(b"acgt"), size=rng.integers(1, 7)).astype(np.uint8)) for _ in range(2)) for _ in range(600)]
    for p, t in pairs:
        assert fc.anchored_distance(fc.anchored(p, 0), fc.anchored(t, 0)) == brute(p, t), (p, t)
    assert fc.anchored_distance(fc.anchored(b"acgt", 0), fc.anchored(b"", 0)) == 4
    assert fc.anchored_distance(fc.anchored(b"", 0), fc.anchored(b"acgt", 0)) == 0


def test_checker_modes_and_matrix_rule():
    assert bytes(b"acgt"[c] for c in fc.anchored(b"aacgT", 0)) == b"aacgt"
    assert bytes(b"acgt"[c] for c in fc.anchored(b"aacgT", 1)) == b"tgcaa"
    assert bytes(b"acgt"[c] for c in fc.anchored(b"aacgT", 2)) == b"ttgca"
    assert bytes(b"acgt"[c] for c in fc.anchored(b"aacgT", 3)) == b"acgtt"
    # three flanks: lengths 4, 6 and 2 (short at min_len 3); reach 5 -> a = 4, 5; the pattern is the shorter one
    pieces = [b"acgt", b"acgtaa", b"ac"]
    a, d = fc.distances(pieces, [0, 1, 2], [0, 0, 0], reach=5, min_len=3)
    assert list(a) == [4, 5, 2]
    assert d.tolist() == [[0, 0, -1], [0, 0, -1], [-1, -1, -1]]
    a, d = fc.distances([b"acgt", b"ttttt"], [0, 1], [0, 0], reach=5, min_len=3)
    assert d[0, 1] == d[1, 0] == brute(b"acgt", b"ttttt") == 3              # (T = 5 bases = min(5, 4 + 1); one 't' matches)


# ---- pfl_neighbours ----
def c_neighbours(piece_read, classes, strands=None):
    from repeatresolver_amd.flanks import neighbours
    return [tuple(int(v) for v in r) for r in zip(*neighbours(piece_read, classes, strands))]


def sda_flanks(piece_read, classes):
    """SDA:226-245 with the read index standing in for the copy: (FlankingLeft, FlankingRight)"""
    msa2seq = [k for k, c in enumerate(classes) if c == "r"]
    unique2seq = [k for k, c in enumerate(classes) if c != "r"]
    seq2reads = list(piece_read)
    right, left = [], []
    for t in range(len(msa2seq)):
        right.append(seq2reads[msa2seq[t]] if msa2seq[t] + 1 in unique2seq and seq2reads[msa2seq[t] + 1] == seq2reads[msa2seq[t]] else -1)
    for t in range(len(msa2seq)):
        left.append(seq2reads[msa2seq[t]] if msa2seq[t] - 1 in unique2seq and seq2reads[msa2seq[t] - 1] == seq2reads[msa2seq[t]] else -1)
    return left, right


# reads: 0 = u r u r u (the middle piece is a right and a left flank); 1 = r u (starts with a row); 2 = u r (ends with one);
# 3 = u r r u (neighbouring rows); 4 = r, 5 = u (a read boundary between a row and a unique piece); 6 = r (the last piece)
HAND_READ = [0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 4, 5, 6]
HAND_CLS = "lrlrl" "rl" "lr" "lrrl" "r" "l" "r"


def test_neighbours_on_hand_made_reads():
    got = c_neighbours(HAND_READ, HAND_CLS)
    assert got == [(1, 0, 1, 2, 0), (3, 2, 1, 4, 0), (5, -1, 1, 6, 0), (8, 7, 1, -1, 0), (10, 9, 1, -1, 0), (11, -1, 1, 12, 0),
                   (13, -1, 1, -1, 0), (15, -1, 1, -1, 0)]
    assert got == fc.neighbours(HAND_READ, HAND_CLS)
    left, right = sda_flanks(HAND_READ, HAND_CLS)
    assert [HAND_READ[r[0]] if r[1] >= 0 else -1 for r in got] == left
    assert [HAND_READ[r[0]] if r[3] >= 0 else -1 for r in got] == right
    assert left == [0, 0, -1, 2, 3, -1, -1, -1] and right == [0, 0, 1, -1, -1, 3, -1, -1]


def test_neighbours_reverse_rows_swap_sides_and_complement():
    strands = [0] * len(HAND_READ)
    for k in (3, 5, 8, 11, 13):
        strands[k] = 1
    got = c_neighbours(HAND_READ, HAND_CLS, strands)
    assert got == fc.neighbours(HAND_READ, HAND_CLS, strands)
    by_piece = {r[0]: r[1:] for r in got}
    assert by_piece[1] == (0, 1, 2, 0)            # forward: left k - 1 backwards, right k + 1 forwards
    assert by_piece[3] == (4, 2, 2, 3)            # reverse: left is k + 1 complemented, right is k - 1 backwards and complemented
    assert by_piece[5] == (6, 2, -1, 3)           # a read that starts with a reverse row has no right flank
    assert by_piece[8] == (-1, 2, 7, 3)
    assert by_piece[11] == (12, 2, -1, 3)         # the row before it is no flank
    assert by_piece[13] == (-1, 2, -1, 3)         # the piece behind belongs to the next read
    rng = np.random.default_rng(2)
    for _ in range(50):                           # random layouts: the C rule is the checker's
        n = int(rng.integers(0, 30))
        reads = np.cumsum(rng.integers(0, 2, size=n)).tolist()
        cls = "".join(rng.choice(["r", "l"], size=n))
        st = rng.integers(0, 2, size=n).tolist()
        assert c_neighbours(reads, cls, st) == fc.neighbours(reads, cls, st)
        if n:
            fwd = c_neighbours(reads, cls)
            left, right = sda_flanks(reads, cls)
            assert [reads[r[0]] if r[1] >= 0 else -1 for r in fwd] == left and [reads[r[0]] if r[3] >= 0 else -1 for r in fwd] == right


# ---- pfl_cluster ----
def matrix(n, edges, short=()):
    d = np.full((n, n), 90, dtype=np.int32)
    for i in range(n):
        d[i, i] = 0
    for i, j, v in edges:
        d[i, j] = d[j, i] = v
    for s in short:
        d[s, :] = -1
        d[:, s] = -1
    return d


def test_cluster_chains_sizes_short_flanks_and_numbering():
    from repeatresolver_amd.flanks import cluster
    a = np.full(7, 100, dtype=np.int32)
    # 5-6 joined, 1-3 and 3-4 joined but 1-4 not (a chain), 0 short, 2 alone
    d = matrix(7, [(5, 6, 40), (1, 3, 40), (3, 4, 40), (1, 4, 90)], short=[0])
    got = cluster(a, d, 400)
    assert got.tolist() == [-1, 0, 1, 0, 0, 2, 2]                       # numbered by lowest member: {1,3,4}, {2}, {5,6}
    assert got.tolist() == fc.cluster(a, d, 400).tolist()
    assert cluster(a, d, 399).tolist() == [-1, 0, 1, 2, 3, 4, 5]        # 1000 * 40 <= 400 * 100 holds, <= 399 * 100 does not
    assert cluster(a, d, 400, min_size=2).tolist() == [-1, 0, -1, 0, 0, 1, 1]
    assert cluster(a, d, 400, min_size=3).tolist() == [-1, 0, -1, 0, 0, -1, -1]
    assert cluster(a, d, 900).tolist() == [-1, 0, 0, 0, 0, 0, 0]
    # the shorter flank's a is the measure: 40 of min(100, 50) is 800 permille
    a2 = a.copy()
    a2[6] = 50
    assert cluster(a2, d, 400).tolist() == [-1, 0, 1, 0, 0, 2, 3]
    assert cluster(np.zeros(0, np.int32), np.zeros((0, 0), np.int32), 400).tolist() == []
    rng = np.random.default_rng(3)
    for _ in range(30):
        n = int(rng.integers(1, 40))
        up = np.triu(rng.integers(0, 120, size=(n, n)), 1)
        dd = (up + up.T).astype(np.int32)
        for s in rng.integers(0, n, size=n // 5):
            dd[s, :] = -1
            dd[:, s] = -1
        aa = rng.integers(100, 257, size=n).astype(np.int32)
        for ms in (1, 2, 4):
            assert cluster(aa, dd, 300, ms).tolist() == fc.cluster(aa, dd, 300, ms).tolist()


# ---- the ABI: declared symbols, refusals, files ----
def test_library_exports_every_symbol_of_pfl_h():
    from repeatresolver_amd import _lib
    text = open(os.path.join(ROOT, "include", "pfl.h")).read()
    declared = set(re.findall(r"\b(pfl_[a-z_]+)\s*\(", text))
    assert declared == set(_lib.PFL_EXPORTS)
    for name in declared:
        assert getattr(lib(), name) is not None
    assert f"#define PFL_MAX_REACH {_lib.PFL_MAX_REACH} " in text and f"#define PFL_MAX_FLANKS {_lib.PFL_MAX_FLANKS} " in text


def test_argument_errors_need_no_device():
    from repeatresolver_amd.flanks import FlankClusterer, cluster, neighbours
    from repeatresolver_amd.realigner import PwrError
    L = lib()
    assert L.pfl_create(None, 0) == -1
    h = ctypes.c_void_p()
    assert L.pfl_create(ctypes.byref(h), -1) == -1
    pi = ctypes.POINTER(ctypes.c_int)
    assert L.pfl_distances(None, 0, None, None, None, None, 256, 100, None, None) == -1
    g = FlankClusterer()                                                # (no device is touched before there is a pair to compute)
    pieces = [b"acgtacgtac", b"acgtacgtaa", b"acgnacgtac"]

    def code(*args, **kw):
        with pytest.raises(PwrError) as e:
            g.distances(*args, **kw)
        return e.value.code
    assert code(pieces, [0, 1], [0, 0], reach=0, min_len=5) == -5
    assert code(pieces, [0, 1], [0, 0], reach=513, min_len=5) == -5
    assert code(pieces, [0, 1], [0, 0], reach=8, min_len=0) == -5
    assert code(pieces, [0, 1], [0, 4], reach=8, min_len=5) == -1
    assert code(pieces, [0, 1], [0, -1], reach=8, min_len=5) == -1
    assert code(pieces, [0, -1], [0, 0], reach=8, min_len=5) == -1
    assert code(pieces, [0, 2], [0, 0], reach=8, min_len=5) == -4       # a byte outside acgtACGT in a listed piece
    assert code(pieces, [0, 2], [0, 0], reach=8, min_len=50) == -4      # also where the flank is short
    lens, dist = g.distances(pieces, [], [], reach=8, min_len=5)        # n == 0
    assert lens.shape == (0,) and dist.shape == (0, 0)
    lens, dist = g.distances(pieces, [1], [3], reach=8, min_len=5)      # one flank: no pair, no device
    assert lens.tolist() == [10] and dist.tolist() == [[0]]
    lens, dist = g.distances(pieces, [0, 1], [0, 0], reach=8, min_len=11)   # all short
    assert lens.tolist() == [10, 10] and dist.tolist() == [[-1, -1], [-1, -1]]
    assert g.stats() == {"cells": 0, "kernel_ms": 0.0}
    g.close()
    with pytest.raises(PwrError) as e:
        cluster([5, 5], [[0, 1], [1, 0]], -1)
    assert e.value.code == -1
    with pytest.raises(PwrError) as e:
        cluster([5, 5], [[0, 1], [1, 0]], 400, min_size=0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        neighbours([0, 0], "r")
    n = ctypes.c_int()
    assert L.pfl_neighbours(-1, None, None, None, ctypes.byref(n), None, None, None, None, None) == -1
    assert L.pfl_neighbours(0, None, None, None, ctypes.byref(n), None, None, None, None, None) == 0 and n.value == 0
    assert L.pfl_labels(None, 0, None, None, None, None, None, 400, 256, 100, 1, ctypes.byref(n), None, None) == -1


def test_info_and_label_files(tmp_path):
    from repeatresolver_amd.flanks import read_info
    L = lib()
    ncut = np.array([2, 0, 1, 0], dtype=np.int32)                       # prc_write_info writes what pfl_read_info reads
    assert L.prc_write_info(str(tmp_path / "info").encode(), 4, ncut.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0
    assert (tmp_path / "info").read_text() == "0 1 2 \n3 \n4 5 \n6 \n"
    assert read_info(tmp_path / "info").tolist() == [0, 0, 0, 1, 2, 2, 3]
    (tmp_path / "empty_read").write_text("0 1 \n\n2 \n")                # a line without a piece still counts as a read
    assert read_info(tmp_path / "empty_read").tolist() == [0, 0, 2]
    (tmp_path / "none").write_text("")
    assert read_info(tmp_path / "none").tolist() == []
    assert read_info(tmp_path / "info", 7).tolist() == [0, 0, 0, 1, 2, 2, 3]
    assert read_info(tmp_path / "info", 9).tolist() == [0, 0, 0, 1, 2, 2, 3, 3, 3]          # the last record's own pieces
    with pytest.raises(ValueError):
        read_info(tmp_path / "info", 6)
    from repeatresolver_amd.realigner import PwrError
    for bad in ("0 2 \n", "1 \n", "0 x \n"):
        (tmp_path / "bad").write_text(bad)
        with pytest.raises(PwrError) as e:
            read_info(tmp_path / "bad")
        assert e.value.code == -4
    with pytest.raises(PwrError) as e:
        read_info(tmp_path / "missing")
    assert e.value.code == -4
    lab = np.array([3, -1, 0, 12], dtype=np.int32)
    assert L.pfl_write_labels(str(tmp_path / "x_FlankingLeft").encode(), 4, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0
    assert (tmp_path / "x_FlankingLeft").read_text() == "3\n-1\n0\n12\n"                   # SDA:248-251
    assert L.pfl_write_labels(str(tmp_path / "no_dir" / "x").encode(), 4, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -8


def test_cli_usage_and_required_threshold(tmp_path):
    import subprocess
    from repeatresolver_amd.flanks import CLI_PATH
    p = subprocess.run([CLI_PATH], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("Usage: ./FlankClusterer Seq.fasta ReadSeqInfo SeqClass -e max_permille\n")
    p = subprocess.run([CLI_PATH, "a", "b", "c"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 1 and "-e max_permille is required" in p.stdout and not os.listdir(tmp_path)
    p = subprocess.run([CLI_PATH, "a_Seq.fasta", "b", "c", "-e", "400"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 1 and not os.listdir(tmp_path)                                   # missing inputs: nothing written
    rr = os.path.join(ROOT, "repeatresolver_amd", "csrc", "RepeatResolver")
    for args in (["-w", "1", "5", "-l", "x"], ["-w", "1", "5", "-r", "x"], ["-f", "1", "5", "-l", "x", "-r", "y"]):
        p = subprocess.run([rr, "no_such_msa"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 1 and "-l and -r go together" in p.stdout and not os.listdir(tmp_path)


# ---- the checker's distances recover the copies ----
@pytest.mark.parametrize("name", ["toy_a", "toy_b"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_checker_distances_cluster_into_the_copies(name, side):
    """flanks of simulate_dataset's true cut, reach 256, min_len 100, max_permille 400: one component per copy, none mixed"""
    from repeatresolver_amd.flanks import cluster
    _pieces, piece, _mode, copy, a, dist = fc.truth_case(name, side)
    label = cluster(a, dist, 400)
    kept = [k for k in range(len(piece)) if dist[k, k] == 0]
    assert all(label[k] == -1 for k in range(len(piece)) if k not in kept) and all(label[k] >= 0 for k in kept)
    copies_of = {}
    for k in kept:
        copies_of.setdefault(int(label[k]), set()).add(copy[k])
    assert all(len(v) == 1 for v in copies_of.values())                                     # no mixed component
    assert len(copies_of) == len({copy[k] for k in kept})                                   # exactly one per copy
    assert label.tolist() == fc.cluster(a, dist, 400).tolist()
